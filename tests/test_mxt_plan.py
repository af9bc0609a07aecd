"""The plan of ltxmi_gemm_mx8_skinny on the CPU (ltxmi_gemm_mx8_skinny_form: the launch's own checks and choice, host arithmetic
only; fake addresses, nothing is dereferenced or launched).

The T5-XXL projections are N = 12288 / 20480 / 4096 with K = 4096 and N = 4096 with K = 10240.  From 256 rows on, the chosen form
must make at least 256 workgroups of every one of them -- one per CU of the MI355X; the 256 x 256 tiles of ltxmi_gemm_mx8 make 16
to 160.  The tile sizes are the header's names for the forms (128 x 64, 64 x 64), restated here."""
import ctypes

import pytest

from test_mx8_abi import BASE, UNSUPPORTED, _gemm

T5_SHAPES = [(12288, 4096), (20480, 4096), (4096, 4096), (4096, 10240)]          # (N, K): qkv, wi, o, wo
ROWS = [64, 128, 256, 512]
TILE = {1: (128, 64), 2: (64, 64)}


def _args(M, N, K, **over):
    kw = dict(M=M, N=N, K=K, lda=K, ldw=K, lda_s=K // 32, ldw_s=K // 32, ldc=N, bias=None)
    kw.update(over)
    return _gemm(False, **kw)


def _form(M, N, K, form=0, **over):
    from ltxmi import _lib
    return _lib.lib.ltxmi_gemm_mx8_skinny_form(ctypes.byref(_args(M, N, K, **over)), form)


def _workgroups(form, M, N):
    bm, bn = TILE[form]
    return -(-M // bm) * -(-N // bn)


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("NK", T5_SHAPES, ids=lambda s: f"N{s[0]}-K{s[1]}")
def test_the_chosen_form_fills_the_chip(NK, M):
    from ltxmi import _lib_mxt
    N, K = NK
    form = _form(M, N, K)
    assert form in _lib_mxt.FORMS, form
    if M >= 256:
        assert _workgroups(form, M, N) >= 256, (form, _workgroups(form, M, N))
    # the residual epilogue (o, wo) plans as the plain one does, and a forced form is the form that runs
    assert _form(M, N, K, epilogue=3, residual=BASE + (5 << 20), ldr=N) == form
    for forced in _lib_mxt.FORMS:
        assert _form(M, N, K, forced) == forced


def test_the_choice_at_the_measured_shapes():
    """profiles/t5_mx8.md: 128 x 64 tiles at 512 rows, 64 x 64 at 256 rows and below."""
    for N, K in T5_SHAPES:
        assert [_form(M, N, K) for M in ROWS] == [2, 2, 2, 1], (N, K)
    assert _form(300, 4096, 4096) == 2              # 3 x 64 tiles of 128 x 64 would leave a quarter of the CUs idle
    assert _form(1, 32, 128) == 2 and _form(512, 288, 128) == 2


def test_a_form_that_does_not_exist_and_rows_above_the_limit_are_refused():
    from ltxmi import _lib, _lib_mxt
    assert _lib_mxt.MAX_ROWS == 512
    for form in (len(_lib_mxt.FORMS) + 1, -1, 64):
        assert _form(256, 4096, 4096, form) == UNSUPPORTED and b"names no tile form" in _lib.lib.ltxmi_last_error()
    for form in (0, *_lib_mxt.FORMS):
        assert _form(_lib_mxt.MAX_ROWS, 4096, 4096, form) > 0
        assert _form(_lib_mxt.MAX_ROWS + 1, 4096, 4096, form) == UNSUPPORTED and b"row limit" in _lib.lib.ltxmi_last_error()
    # what the shared checks refuse is refused by the plan as well: it is the launch's own check
    assert _form(256, 4096, 4096 + 64) == UNSUPPORTED and b"multiple of 128" in _lib.lib.ltxmi_last_error()


def test_the_ring_fits_the_lds():
    """Stage bytes as csrc/gemm_mx8_skinny.hip lays them out: (BM + 64) rows of 128 bytes and 1 KiB of scale words."""
    from ltxmi import _lib_mxt
    lds = 160 * 1024
    for form, (bm, bn) in TILE.items():
        assert _lib_mxt.STAGES * ((bm + bn) * 128 + 1024) <= lds // (1 if form == 1 else 2)
