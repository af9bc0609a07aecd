"""One keyed cache for tensors derived from other tensors: packed weights, expanded tables, the step-invariant projections.

What a key sees, per source tensor: address, version counter, dtype, device, shape and stride.  A reload or a cast gives a
new address; an in-place edit that autograd sees (``weight.copy_``, ``+=``, ``add_`` -- what a LoRA merge does) a new
version; a view of the same storage another shape or stride.  What it can NOT see: an edit through ``.data`` (it bumps no
counter) and any edit of an inference tensor (created, loaded or cast under ``torch.inference_mode()``: it has no counter,
``tensor_version`` gives -1).  After those call ``invalidate_packed()`` on the module that owns the cache.  An address
stands for its tensor only while that tensor is alive, so every entry holds its sources: an address in a live key cannot
be handed to another tensor.

This module imports neither ``ops`` nor the library."""
import torch


def tensor_version(t):
    """``t._version``, or -1 for an inference tensor (it tracks none and raises on the read)."""
    try:
        return t._version
    except RuntimeError:
        return -1


def cache_key(sources, extras=(), layout=True):
    """The key of a value derived from ``sources`` (tensors, or None where a module has none, e.g. no bias) and of the
    non-tensor ``extras`` it depends on (a slot name, a layout switch, a length, an adapter epoch).  ``layout=False`` leaves
    shape and stride out: for sources that are parameters or packs, whose layout at one address and version is fixed, while
    a caller's prompt or mask may be another view of the same storage (a row slice that starts at row 0)."""
    if layout:
        return (*[None if t is None else (t.data_ptr(), tensor_version(t), t.dtype, t.device, t.shape, t.stride())
                  for t in sources], *extras)
    return (*[None if t is None else (t.data_ptr(), tensor_version(t), t.dtype, t.device) for t in sources], *extras)


class DerivedCache:
    """Up to ``capacity`` derived values; full means cleared, as a generation's few prompts and masks come and go together."""
    __slots__ = ("capacity", "layout", "_entries")

    def __init__(self, capacity=1, layout=True):
        self.capacity, self.layout, self._entries = capacity, layout, {}

    def get(self, sources, extras, build, enabled=True):
        """The value for (sources, extras); ``build()`` makes it on a miss.  ``enabled=False``: build, keep nothing."""
        if not enabled:
            return build()
        key = cache_key(sources, extras, self.layout)
        hit = self._entries.get(key)
        if hit is None:
            hit = self.put(sources, extras, build(), key)
        return hit[0]

    def put(self, sources, extras, value, key=None):
        """Seed the entry of (sources, extras) with a value made elsewhere."""
        if len(self._entries) >= self.capacity:
            self._entries.clear()
        hit = self._entries[key or cache_key(sources, extras, self.layout)] = (value, tuple(sources))
        return hit

    def clear(self):
        self._entries.clear()

    def __len__(self):
        return len(self._entries)


class DerivedOwner:
    """Mixin (before ``nn.Module`` in the bases) for a module that derives tensors from its parameters: named caches made on
    first use, dropped by ``invalidate_packed()``, by ``.to()`` / ``.cuda()`` / ``.half()`` and by ``load_state_dict``."""

    def derived(self, slot, capacity=1, layout=False):
        """The cache named ``slot``; ``layout=True`` where a source is not this module's (``cache_key``)."""
        try:
            return self.__dict__["_derived"][slot]
        except KeyError:
            return self.__dict__.setdefault("_derived", {}).setdefault(slot, DerivedCache(capacity, layout))

    def derived_slots(self):
        """Names of the caches that hold a value."""
        return {slot for slot, cache in self.__dict__.get("_derived", {}).items() if len(cache)}

    def invalidate_packed(self):
        """Drop this module's derived values (rebuilt on next use); needed after edits a key cannot see (module docstring)."""
        self.__dict__.pop("_derived", None)

    def _apply(self, fn, *a, **k):
        self.invalidate_packed()
        return super()._apply(fn, *a, **k)

    def _load_from_state_dict(self, *a, **k):
        self.invalidate_packed()
        return super()._load_from_state_dict(*a, **k)

    def _packed_linears(self, slot, mods):
        """Contiguous [sum(out), in] weight (and bias, or None) of the linears ``mods``: one GEMM operand, cached as ``slot``."""
        def build():
            with torch.no_grad():
                w = torch.cat([m.weight for m in mods], dim=0).contiguous()
                b = torch.cat([m.bias for m in mods], dim=0).contiguous() if mods[0].bias is not None else None
            return w, b
        return self.derived(slot).get([t for m in mods for t in (m.weight, m.bias)], (), build)
