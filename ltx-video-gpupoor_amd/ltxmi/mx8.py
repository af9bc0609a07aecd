"""MX-FP8 in plain torch, for tools and tests; never on the product path (the kernels are ops.quantize_mx8 / ops.gemm_mx8).

The format (include/ltxmi_mx.h): blocks of 32 consecutive elements of a row share one E8M0 scale byte (value 2^(byte - 127));
the elements are OCP e4m3fn."""
import torch

BLOCK = 32
E4M3 = torch.float8_e4m3fn


def dequantize(q, scales, dtype=torch.float32):
    """q [..., K] (float8_e4m3fn, or its uint8 bytes), scales [..., K / 32] uint8 -> q * 2^(scales - 127) as ``dtype``.
    Exact in float32 and float64 (a product by a power of two), except that float32 flushes nothing but loses the bits of a
    result below 2^-149."""
    if q.dtype == torch.uint8:
        q = q.view(E4M3)
    if q.dtype != E4M3 or scales.dtype != torch.uint8:
        raise TypeError(f"ltxmi.mx8.dequantize: expected float8_e4m3fn (or uint8) elements and uint8 scales, got {q.dtype}, {scales.dtype}")
    if q.shape[-1] != scales.shape[-1] * BLOCK or q.shape[:-1] != scales.shape[:-1]:
        raise ValueError(f"ltxmi.mx8.dequantize: q {tuple(q.shape)} and scales {tuple(scales.shape)} do not belong together")
    e = (scales.to(torch.int32) - 127).repeat_interleave(BLOCK, dim=-1)
    return torch.ldexp(q.to(dtype), e)
