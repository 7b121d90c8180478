"""Host side of the HIP rendering path: tensor plumbing around the C ABI (include/enslam_hip.h).

PyTorch is used for device memory, streams and autograd bookkeeping only; every arithmetic step of the
path (sampling, gather, decoders, compositing and their backward) runs in libenslam_hip.so.
There is no CPU implementation here: non-HIP tensors raise.
"""
import ctypes
import os
import weakref

import torch

from . import _lib as L
from .event import EVENTNET_CONVS

_KIND_OF_GRID = {'grid_coarse': 0, 'grid_middle': 1, 'grid_fine': 2, 'grid_color': 3}


def _require_hip(t, what):
    if not t.is_cuda:
        raise L.EnslamError(f"{what} must live on a HIP device (got {t.device}); the rendering path has no CPU "
                            f"fallback")


def engine_on_calling_thread():
    """Context manager: run the backward passes started inside it on the calling thread instead of the autograd engine's
    per-device worker thread.  For a Python-implemented autograd.Function the worker thread costs two thread switches and a
    GIL hand-over per call (0.25-0.3 ms of a 0.9 ms Python-driven step, tools/hostprof.py); results are identical.  The
    switch is scoped: PyTorch's setting is restored on exit and nothing outside the block changes (round 3 flipped it
    process-wide in Renderer.__init__).  `ENSLAM_KEEP_AUTOGRAD_THREADS=1` makes this a no-op.

        with EF.engine_on_calling_thread():
            loss.backward()
    """
    if os.environ.get('ENSLAM_KEEP_AUTOGRAD_THREADS') == '1':
        import contextlib
        return contextlib.nullcontext()
    return torch.autograd.set_multithreading_enabled(False)


# ---- tensors another PROCESS writes ---------------------------------------------------------------------------------
# The cached device-side forms (voxel-major copies of contiguous grids, packed decoders) are keyed on (tensor identity,
# _version).  `_version` is a counter of THIS process's tensor object: an in-place update made by another process on the same
# device memory (the reference shares its map and decoders between three processes over CUDA IPC: EvenNICER_SLAM.py:75-95,
# 313-332) does not move it.  The reference's own flow never renders such memory directly -- the tracker clones the map and
# deep-copies the decoders every frame (Tracker.py:248-260), the mappers render the tensors they themselves update
# (Mapper.py:633-641) -- and is safe as it stands.  A caller that DOES render straight from memory another process writes
# declares it: `external_writers(True)` (or ENSLAM_EXTERNAL_WRITERS=1) makes every version-keyed cache miss, so each call
# re-converts the touched blocks and re-packs the decoders from what the memory holds now (channels_last_3d grids are read in
# place and are current either way).  tests/test_hip_multiprocess.py exercises all of it across spawned processes.
_external = [os.environ.get('ENSLAM_EXTERNAL_WRITERS') == '1', 0]


def external_writers(on=True):
    """Declare that tensors handed to the renderer may be modified in place by other processes (see above); returns the
    previous setting."""
    prev, _external[0] = _external[0], bool(on)
    return prev


def _ver(t):
    """Version of tensor t for cache keys: its `_version`, or -- with external writers declared -- a value no cache has seen."""
    if _external[0]:
        _external[1] += 1
        return -_external[1]
    return t._version


def _live_grid_guard(grids):
    """[(grid, version)] of the channels_last_3d grids a render call reads IN PLACE: its backward reads the same storage again
    (corner re-gather of the ray gradients, the recompute route), through a detached alias autograd does not version-check."""
    return [(g, g._version) for g in grids if is_native_grid(g)]


def _check_live_grids(guard):
    """Plain torch raises when a tensor saved for backward has been modified in place; the in-place read of a native grid gets
    the same protection: an optimiser step / MaskedGridOptimizer.step / any in-place write to the map between a render call
    and its backward would silently give ray and grid gradients of a different map."""
    for g, v in guard:
        if g._version != v:
            raise L.EnslamError("a feature grid read in place by this render call (channels_last_3d layout) was modified in place "
                                f"between the call and its backward (version {v} -> {g._version}): backpropagate before updating "
                                "the map, or render from a clone")


def _f32c(t):
    """detached contiguous float32 form of t (no copies, no dispatcher calls beyond detach() when it already is one)."""
    t = t.detach()
    if t.dtype is not torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _stream():
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


def _ptr(t):
    """Device address of t as a plain int (None -> NULL): ctypes converts both for c_void_p parameters, and an int costs a
    quarter of a c_void_p object (a colour-stage step passes ~180 addresses)."""
    return t.data_ptr() if t is not None else None


def _ptrv(t):
    return t.data_ptr() if t is not None else 0


# ------------------------------------------------------------------------------------------------
# hipGraph capture bookkeeping (graph.GraphedStep)
# ------------------------------------------------------------------------------------------------
# Cached device-side forms (voxel-major grids, packed decoders) that are CREATED while a stream capture is recording live
# in the graph's private memory pool and only hold data once that graph has been replayed; every replay rewrites them
# with the values its inputs had at the START of the replay.  They are therefore tagged with the capture they were made
# in and are invisible to everything outside that capture (an eager render after replays re-packs from the live tensors).
_capture = {'epoch': 0, 'active': 0, 'raw_writes': None, 'init_zero': None, 'persist': None, 'persist_need': {}}

# Persistent dense gradients of captured steps (see _RenderFn.backward): data_ptr of the gradient buffer -> the uint8 flags of
# the 64-voxel blocks that hold non-zeros (`prev` of enslam_step_finish_rays_prev).  The finish launch of the next replay
# rewrites exactly the blocks flagged here or touched by its own rays, so EVERY other writer of such a buffer has to add the
# blocks it fills to these flags: parallel.allreduce_gradients (the sums of the other ranks' blocks) does through
# note_foreign_blocks().  Entries live as long as the GraphedStep that captured them (graph.GraphedStep.close / __del__).
# An address alone does not identify a buffer (the allocator hands a freed address out again): an entry is
# data_ptr -> (the buffer's STORAGE, flags).  The entry holds the storage (so its address cannot be handed out again while the
# entry lives) but not the tensor: a second reference to the tensor would make AccumulateGrad clone the gradient instead of
# adopting it, and the `.grad` that callers pass back in is a detached alias (another tensor object on the same storage)
# anyway.  A look-up compares the storage; a graph that goes away removes only the entries that are still its own
# (_persist_register / forget_persistent).
_persist_prev = {}


def _persist_register(g, pv):
    _persist_prev[g.data_ptr()] = (g.untyped_storage(), pv)


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _cap_tag():
    """0 outside a capture, else the id of the capture being recorded.  (graph.GraphedStep announces its capture through
    begin_capture(): without one no stream query is made -- six of them cost 25 us of a Python-driven step.)"""
    if not _capture['active']:
        return 0
    return _capture['active'] if _capturing() else 0


def _tag_visible(tag):
    return tag == 0 or tag == _cap_tag()


def begin_capture():
    """Called by graph.GraphedStep right before it starts recording: new capture id, fresh log of raw writes.
    One capture at a time per process: the bookkeeping is process-wide (hipGraph capture itself is per stream, but the caches
    tagged here are shared), so a second capture started before the first has ended is refused instead of mixing their logs."""
    if _capture['active']:
        raise L.EnslamError("a hipGraph capture of this library is already being recorded in this process (captures do not nest "
                            "and cannot run on two threads at once)")
    _capture['epoch'] += 1
    _capture['active'] = _capture['epoch']
    _capture['raw_writes'] = []
    _capture['init_zero'] = []
    _capture['persist'] = {}          # id(grid) -> (gradient data_ptr, prev flags) of this capture
    _capture['persist_need'] = {}     # id(grid) -> the flags this step's sampler marks (persistent native gradients)


def end_capture(ok=True):
    """-> the tensors that kernels of the captured step write behind torch's back (note_raw_write).  ok=False: the capture
    raised -- its storages belong to a pool that is being torn down, nothing is touched (and nothing here may hide the
    original exception)."""
    log, _capture['raw_writes'] = _capture['raw_writes'] or [], None
    _capture['active'] = 0
    # persistent gradient tensors of the captured step and their block flags (see _RenderFn.backward): the protocol starts
    # from all-zero memory; filled here, eagerly, once -- a fill inside the capture would run at every replay
    init, _capture['init_zero'] = _capture['init_zero'] or [], None
    if not ok:
        forget_persistent(list((_capture['persist'] or {}).values()))
        _capture['persist'] = None
        _capture['persist_need'] = {}
        end_capture.persist_keys = []
        return []
    for storage in init:
        torch.empty(0, dtype=torch.uint8, device=storage.device).set_(storage).zero_()
    seen, out = set(), []
    for t in log:
        if id(t) not in seen:
            seen.add(id(t))
            out.append(t)
    persist, _capture['persist'] = _capture['persist'] or {}, None
    _capture['persist_need'] = {}
    end_capture.persist_keys = list(persist.values())                      # (ptr, flags) pairs, read by graph.GraphedStep
    return out


def forget_persistent(keys):
    """The graph that owned these persistent gradient buffers is gone (graph.GraphedStep.close): keys = its (data_ptr, flags)
    pairs.  Only entries that still carry THESE flags are removed -- a newer graph may have been given the same address."""
    for ptr, pv in keys:
        e = _persist_prev.get(ptr)
        if e is not None and e[1] is pv:
            del _persist_prev[ptr]


def note_foreign_blocks(grad, flags):
    """`grad` (a dense feature-grid gradient) has just been written in the 64-voxel blocks flagged in `flags` (uint8, one per
    block) by something other than the render backward -- the unpack of a gradient all-reduce.  If it is the persistent
    gradient buffer of a captured step, those blocks join the flags of the blocks its next replay must rewrite."""
    e = _persist_prev.get(grad.data_ptr())
    if e is None:
        return False
    st0, pv = e
    if st0._cdata != grad.untyped_storage()._cdata:     # another buffer at the same address
        return False
    if pv.numel() == flags.numel():
        torch.maximum(pv, flags.reshape(pv.shape).to(pv.dtype), out=pv)
        return True
    return False


def note_raw_write(tensors):
    """A library kernel is about to overwrite these tensors in place (mapper.FusedAdam, MaskedGridOptimizer): bump their
    version counters so the caches keyed on `_version` miss, and -- under capture -- remember them so that every replay
    of the graph bumps them again (the Python call itself only runs at capture time)."""
    torch._C._increment_version(list(tensors))      # (a LIST: handed a tensor, the call iterates over its rows -- 25 us each)
    if _capture['raw_writes'] is not None and _capturing():
        _capture['raw_writes'].extend(tensors)


_bound6_cache = {}


def bound6(bound):
    """[3,2] tensor -> (c_double*6) x_lo,x_hi,y_lo,y_hi,z_lo,z_hi.  Cached per (tensor identity, version): a scene's bound is
    set once (EvenNICER_SLAM.load_bound) and read by every render call."""
    key = id(bound)
    hit = _bound6_cache.get(key)
    if hit is not None and hit[0]() is bound and hit[1] == bound._version:
        return hit[2]
    b = bound.detach().to('cpu', torch.float64).reshape(-1).tolist()
    out = (ctypes.c_double * 6)(*b)
    if len(_bound6_cache) > 64:
        _bound6_cache.clear()
    _bound6_cache[key] = (weakref.ref(bound), bound._version, out)
    return out


# ------------------------------------------------------------------------------------------------
# decoder parameters: ordering, packing cache
# ------------------------------------------------------------------------------------------------
_layer_cache = weakref.WeakKeyDictionary()     # decoder module -> its Linear sub-modules (+ embedder), ABI order


def decoder_params(dec, kind):
    """Parameter tensors of one decoder in ABI order.  Works on this package's modules and on any
    module with the reference's attribute names (pts_linears, fc_c, output_linear, embedder._B).
    The sub-module list is cached (nn.ModuleList indexing is slow); parameters are re-read every call."""
    mods = _layer_cache.get(dec)
    if mods is None:
        mods = [dec.pts_linears[i] for i in range(5)]
        if kind != L.MLP_COARSE:
            mods += [dec.fc_c[i] for i in range(5)]
        mods.append(dec.output_linear)
        _layer_cache[dec] = mods
    ps = []
    for m in mods:
        p = m._parameters
        ps.append(p['weight'])
        ps.append(p['bias'])
    if kind != L.MLP_COARSE:
        ps.append(dec.embedder._B)
    return ps


_flat_offsets = {}


def _flat_params_struct(kind, like, base):
    """enslam_mlp_params of tensors laid out back to back (float32) from address `base` in decoder_params() order with the
    sizes of `like` -> (struct, address behind the last one).  The byte offsets are cached per (kind, sizes)."""
    key = (kind, tuple(t.numel() for t in like))
    offs = _flat_offsets.get(key)
    if offs is None:
        o, offs = 0, []
        for n in key[1]:
            offs.append(o)
            o += 4 * n
        offs.append(o)
        _flat_offsets[key] = offs = tuple(offs)
    s = L.MlpParams()
    it = iter(offs)
    for i in range(5):
        s.W[i] = base + next(it)
        s.b[i] = base + next(it)
    if kind != L.MLP_COARSE:
        for i in range(5):
            s.Wc[i] = base + next(it)
            s.bc[i] = base + next(it)
    s.Wo = base + next(it)
    s.bo = base + next(it)
    if kind != L.MLP_COARSE:
        s.B = base + next(it)
    return s, base + offs[-1]


def _fill_params_struct(kind, tensors):
    """enslam_mlp_params from tensors in decoder_params() order (entries may be None)."""
    s = L.MlpParams()
    it = iter(tensors)
    for i in range(5):
        s.W[i] = _ptrv(next(it))
        s.b[i] = _ptrv(next(it))
    if kind != L.MLP_COARSE:
        for i in range(5):
            s.Wc[i] = _ptrv(next(it))
            s.bc[i] = _ptrv(next(it))
    s.Wo = _ptrv(next(it))
    s.bo = _ptrv(next(it))
    if kind != L.MLP_COARSE:
        s.B = _ptrv(next(it))
    return s


_EXPECT_SHAPES = {
    L.MLP_COARSE: [(32, 32), (32,), (32, 32), (32,), (32, 32), (32,), (32, 64), (32,), (32, 32), (32,), (1, 32), (1,)],
}


def _xyz_shapes(cd, nout):
    s = []
    for k in (93, 32, 32, 125, 32):
        s += [(32, k), (32,)]
    for _ in range(5):
        s += [(32, cd), (32,)]
    return s + [(nout, 32), (nout,), (3, 93)]


_EXPECT_SHAPES[L.MLP_MIDDLE] = _xyz_shapes(32, 1)
_EXPECT_SHAPES[L.MLP_FINE] = _xyz_shapes(64, 1)
_EXPECT_SHAPES[L.MLP_COLOR] = _xyz_shapes(32, 4)


def _check_params(kind, ps):
    for t, shp in zip(ps, _EXPECT_SHAPES[kind]):
        if tuple(t.shape) != shp or t.dtype != torch.float32 or not t.is_contiguous():
            raise L.EnslamError(f"decoder {L.MLP_NAMES[kind]}: parameter of shape {tuple(t.shape)} / {t.dtype}, "
                                f"expected contiguous float32 {shp}")
        _require_hip(t, "decoder parameters")


_ELEM_SIZE = {torch.uint8: 1, torch.int32: 4, torch.float32: 4, torch.float64: 8, torch.int64: 8}
_size_memo = {}


def _lib_size(name, *args):
    """Memoised size queries of the library (enslam_packed_floats & co.: pure functions of small integers)."""
    key = (name,) + args
    v = _size_memo.get(key)
    if v is None:
        v = _size_memo[key] = int(getattr(L.lib(), name)(*args))
    return v


class _ZeroArena:
    """One zero-filled allocation per render call, handed out in aligned typed slices (block flags, validity
    bitmaps, packed-decoder buffers): one fill node in the step's graph instead of one per consumer."""

    def __init__(self, device, nbytes, persistent=False):
        # persistent (inside a captured training step, see _RenderFn.forward): no fill node -- the memory is the same at
        # every replay, zeroed once by end_capture(), and every slice handed out is back to zero (or wholly rewritten) when
        # the step ends.  Allocated at the first take(): a call that needs nothing zeroed (tracker iterations on a cached
        # map) gets no fill node either.
        self.device, self.nbytes, self.persistent = device, max(int(nbytes), 16), persistent
        self.buf = None
        self.off = 0

    def _alloc(self):
        if self.persistent:
            self.buf = torch.empty(self.nbytes, dtype=torch.uint8, device=self.device)
            _capture['init_zero'].append(self.buf.untyped_storage())
        else:
            self.buf = torch.zeros(self.nbytes, dtype=torch.uint8, device=self.device)

    def take(self, n, dtype):
        if self.buf is None:
            self._alloc()
        nb = n * _ELEM_SIZE[dtype]
        off = (self.off + 15) & ~15
        if off + nb > self.buf.numel():
            return torch.zeros(n, dtype=dtype, device=self.buf.device)
        self.off = off + nb
        return self.buf[off:off + nb].view(dtype)


class _PackCache:
    """Packed form of a decoder, refreshed when any parameter's (data_ptr, _version) changes."""

    def __init__(self):
        self.key = None
        self.packed = None
        self.tag = 0            # capture the packing was made in (0: eager memory)

    def fresh(self, key):
        return key == self.key and self.packed is not None and _tag_visible(self.tag)

    def get(self, kind, ps):
        key = _params_key(self, ps)
        if not self.fresh(key):
            _check_params(kind, ps)
            n = L.lib().enslam_packed_floats(kind)
            # fresh buffer: an earlier forward's saved packing stays valid for its backward
            packed = torch.zeros(n, dtype=torch.float32, device=ps[0].device)
            s = _fill_params_struct(kind, ps)
            L.check(L.lib().enslam_pack_mlp(kind, ctypes.byref(s), _ptr(packed), _stream()), "enslam_pack_mlp")
            self.key, self.packed, self.tag = key, packed, _cap_tag()       # (only after the launch was accepted)
        return self.packed


_pack_caches = weakref.WeakKeyDictionary()      # decoder module -> _PackCache


def _params_key(cache, ps):
    """Cache key of a decoder's parameter list: (id, data_ptr, _version) per tensor -- 69 x 3 attribute reads per colour-stage
    call when built naively.  While the list holds the SAME tensor objects as the previous call (the normal case: a module's
    parameters) only the version counters and the storage addresses are re-read, and the address part of the previous key is
    reused when none moved (an optimiser step changes versions, never storage)."""
    prev = getattr(cache, 'ps_seen', None)
    if prev is not None and len(prev) == len(ps) and all(a is b for a, b in zip(prev, ps)):
        ptrs = tuple(p.data_ptr() for p in ps)
        if ptrs == cache.ptrs_seen:
            return (cache.ids_seen, ptrs, tuple(_ver(p) for p in ps))
    cache.ps_seen = list(ps)
    cache.ids_seen = tuple(id(p) for p in ps)
    cache.ptrs_seen = tuple(p.data_ptr() for p in ps)
    return (cache.ids_seen, cache.ptrs_seen, tuple(_ver(p) for p in ps))


def packed_decoders(items, arena=None, defer=False):
    """Packed forms of several decoders [(module, kind, params)]; stale ones are rebuilt with ONE zero-fill and ONE
    launch (up to three decoders per launch).  defer=True (at most three stale decoders): nothing is launched, the
    second return value holds the arguments (n, kinds, structs, ptrs) for enslam_step_prepare, or None, and the third
    a `commit()` the caller invokes once that launch has been accepted -- a cache entry is only marked fresh then, so a
    failure in between (allocation, a refused launch) cannot leave a "fresh" entry pointing at a zero-filled buffer."""
    out, stale = [], []
    for i, (dec, kind, ps) in enumerate(items):
        cache = _pack_caches.get(dec)
        if cache is None:
            cache = _pack_caches[dec] = _PackCache()
        key = _params_key(cache, ps)
        if cache.fresh(key):
            out.append(cache.packed)
        else:
            out.append(None)
            stale.append((i, cache, key))
    pending = []

    def commit():
        tag = _cap_tag()
        for cache, key, packed in pending:
            cache.key, cache.packed, cache.tag = key, packed, tag
        del pending[:]

    if stale:
        lib = L.lib()
        sizes = [_lib_size('enslam_packed_floats', items[i][1]) for i, _, _ in stale]
        flat = (arena.take(sum(sizes), torch.float32) if arena is not None else
                torch.zeros(sum(sizes), dtype=torch.float32, device=items[stale[0][0]][2][0].device))
        pieces = flat.split(sizes)
        for j, (i, cache, key) in enumerate(stale):
            # an optimiser step changes versions, not storage: the shape checks and the pointer struct of unchanged
            # storages are reused (they are half of the host cost of a re-pack)
            where = key[:2]
            if where != getattr(cache, 'where', None):
                _check_params(items[i][1], items[i][2])
                cache.where, cache.struct = where, _fill_params_struct(items[i][1], items[i][2])
            pending.append((cache, key, pieces[j]))
            out[i] = pieces[j]
        deferred = None
        for g0 in range(0, len(stale), 3):
            grp = stale[g0:g0 + 3]
            n = len(grp)
            kinds, structs, ptrs = (ctypes.c_int32 * n)(), (L.MlpParams * n)(), (ctypes.c_void_p * n)()
            for j, (i, cache, key) in enumerate(grp):
                kinds[j] = items[i][1]
                structs[j] = cache.struct
                ptrs[j] = out[i].data_ptr()
            if defer and len(stale) <= 3:
                deferred = (n, kinds, structs, ptrs)
            else:
                L.check(lib.enslam_pack_mlp_multi(n, kinds, structs, ptrs, _stream()), "enslam_pack_mlp_multi")
        if defer:
            if deferred is None:
                commit()
            return out, deferred, commit
        commit()
    elif defer:
        return out, None, commit
    return out


def packed_decoder(dec, kind, params=None):
    cache = _pack_caches.get(dec)
    if cache is None:
        cache = _pack_caches[dec] = _PackCache()
    return cache.get(kind, params if params is not None else decoder_params(dec, kind))


# ------------------------------------------------------------------------------------------------
# grids: voxel-major copies, cached per (storage, version)
# ------------------------------------------------------------------------------------------------
class _GridEntry:
    __slots__ = ('ref', 'version', 'vm', 'valid', 'tag')

    def __init__(self, ref, version, vm, valid, tag):
        self.ref, self.version, self.vm, self.valid, self.tag = ref, version, vm, valid, tag


def _check_grid(g):
    if g.dim() != 5 or g.shape[0] != 1 or g.shape[1] != 32 or g.dtype != torch.float32:
        raise L.EnslamError(f"feature grid must be float32 [1,32,D,H,W], got {tuple(g.shape)} {g.dtype}")
    _require_hip(g, "feature grids")


_CL3D = torch.channels_last_3d


def is_native_grid(g):
    """A feature grid whose storage already is the kernels' own [V][32] layout: a [1,32,D,H,W] tensor in torch's
    channels_last_3d memory format (`grid.contiguous(memory_format=torch.channels_last_3d)` -- same shape, same values, same
    indexing as the reference's grids; only the strides differ).  Such a grid is gathered from where it lies, nothing is
    converted per step, and its gradient comes back in the same memory format without a transposed copy."""
    return (g.dim() == 5 and g.shape[1] == 32 and g.is_contiguous(memory_format=_CL3D) and not g.is_contiguous()
            and g.data_ptr() % 16 == 0)           # (the gathers load 16 bytes at a time: an odd view offset takes the copying route)


def _native_vm(g):
    """[V,32] view of a native grid's storage."""
    return g.detach().permute(0, 2, 3, 4, 1).reshape(-1, 32)


def _native_grad_view(flat, dims):
    """[1,32,D,H,W] channels_last_3d tensor over a flat [V*32] gradient buffer."""
    D, H, W = dims
    return flat.view(1, D, H, W, 32).permute(0, 4, 1, 2, 3)


class _GridCache:
    """Voxel-major copies keyed on tensor IDENTITY + version counter.  (A data_ptr key would go stale when the
    caching allocator hands a freed grid's address to a new tensor, e.g. Tracker.update_para_from_mapping's
    per-frame clones.)  Entries die with their source tensor.  An entry is either dense (every voxel converted,
    `valid is None`) or sparse (`valid` = bitmap of the 64-voxel blocks converted so far); entries made while a
    hipGraph capture records are only visible inside that capture (see _capture)."""

    def __init__(self):
        self.items = {}          # id(tensor) -> _GridEntry

    def _lookup(self, g, sparse):
        e = self.items.get(id(g))
        if e is not None and e.ref() is g and e.version == _ver(g) and (e.valid is not None) == sparse and _tag_visible(e.tag):
            return e
        return None

    def _store(self, g, vm, valid):
        key, items = id(g), self.items
        items[key] = _GridEntry(weakref.ref(g, lambda _r, key=key, items=items: items.pop(key, None)), g._version, vm, valid,
                                _cap_tag())

    def get(self, g):
        _check_grid(g)
        if is_native_grid(g):
            return _native_vm(g)
        e = self._lookup(g, False)
        if e is not None:
            return e.vm
        src = g.detach()
        if not src.is_contiguous():
            src = src.contiguous()
        V = g.shape[2] * g.shape[3] * g.shape[4]
        # fresh buffer each refresh: an earlier forward's saved copy stays valid for its backward
        vm = torch.empty((V, 32), dtype=torch.float32, device=g.device)
        L.check(L.lib().enslam_grid_to_voxel_major(_ptr(src), _ptr(vm), V, _stream()), "grid_to_voxel_major")
        self._store(g, vm, None)
        return vm

    def get_many(self, grids):
        """Voxel-major copies of several grids; all cache misses are converted in ONE launch."""
        out, miss = [], []
        for i, g in enumerate(grids):
            if is_native_grid(g):
                _check_grid(g)
                out.append(_native_vm(g))
                continue
            e = self._lookup(g, False)
            out.append(e.vm if e is not None else None)
            if e is None:
                miss.append(i)
        if len(miss) == 1:
            out[miss[0]] = self.get(grids[miss[0]])
        elif miss:
            n = len(miss)
            srcs, dsts, vs, keep = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)(), (ctypes.c_int64 * n)(), []
            for j, i in enumerate(miss):
                g = grids[i]
                _check_grid(g)
                src = g.detach()
                src = src if src.is_contiguous() else src.contiguous()
                V = g.shape[2] * g.shape[3] * g.shape[4]
                vm = torch.empty((V, 32), dtype=torch.float32, device=g.device)
                srcs[j], dsts[j], vs[j] = src.data_ptr(), vm.data_ptr(), V
                keep.append(src)
                out[i] = vm
            L.check(L.lib().enslam_grids_convert(n, srcs, dsts, vs, 1, _stream()), "enslam_grids_convert")
            for i in miss:
                self._store(grids[i], out[i], None)
        return out

    def get_many_sparse(self, grids, need, arena=None, defer=False, fresh=False):
        """Voxel-major copies in which (at least) the 64-voxel blocks flagged in need[i] (uint8 tensors) are valid.
        Every entry carries a `valid` bitmap; one launch converts the blocks that are needed and not yet valid.
        fresh: no bitmap and no cache entry -- every flagged block is converted by this call's launch (a captured
        training step: the grids change between replays, and a bitmap would have to be cleared at every replay)."""
        n = len(grids)
        srcs, dsts, vs = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)(), (ctypes.c_int64 * n)()
        needs, valids, out, keep = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)(), [], []
        for i, g in enumerate(grids):
            e = None if fresh else self._lookup(g, True)
            if fresh:
                _check_grid(g)
                V = g.shape[2] * g.shape[3] * g.shape[4]
                vm, valid = torch.empty((V, 32), dtype=torch.float32, device=g.device), None
            elif e is not None:
                vm, valid = e.vm, e.valid
            else:
                _check_grid(g)
                V = g.shape[2] * g.shape[3] * g.shape[4]
                vm = torch.empty((V, 32), dtype=torch.float32, device=g.device)
                valid = (arena.take((V + 63) // 64, torch.uint8) if arena is not None else
                         torch.zeros((V + 63) // 64, dtype=torch.uint8, device=g.device))
                self._store(g, vm, valid)
            src = g.detach()
            src = src if src.is_contiguous() else src.contiguous()
            keep.append(src)
            srcs[i], dsts[i], vs[i] = src.data_ptr(), vm.data_ptr(), vm.shape[0]
            needs[i], valids[i] = need[i].data_ptr(), (valid.data_ptr() if valid is not None else None)
            out.append(vm)
        if defer:                    # the caller launches (enslam_step_prepare); `keep` pins the sources until then
            return out, (n, srcs, dsts, vs, needs, valids, keep)
        L.check(L.lib().enslam_grids_convert_sparse(n, srcs, dsts, vs, needs, valids, 1, _stream()),
                "enslam_grids_convert_sparse")
        return out


_grid_cache = _GridCache()


def clear_caches():
    _grid_cache.items.clear()
    _pack_caches.clear()


def refresh_in_place(c, decoders, stage='color'):
    """Bring the cached device-side forms of a map up to date IN PLACE after its tensors were updated in place
    (`Tracker.update_para_from_mapping` copying the mapper's state into the tracker's tensors, an optimiser step):
    the voxel-major copies of dense no-gradient grids and the packed decoders are rewritten inside their existing
    buffers.  A captured step (graph.GraphedStep, tracker.GraphedCameraIteration) that was recorded while those caches
    were warm contains no conversion / packing launch and reads exactly these buffers, so this call is what makes it
    see the new map.  Must not run between a forward and its backward.  Returns the number of buffers rewritten."""
    lib = L.lib()
    n = 0
    for k in stage_kinds(stage):
        g = c[L.GRID_NAMES[k]]
        if isinstance(g, VoxelMajorGrid):
            continue                                    # already the kernels' layout: nothing cached
        e = _grid_cache.items.get(id(g))
        if e is not None and e.ref() is g and e.valid is None and e.tag == 0 and e.version != g._version:
            src = g.detach()
            src = src if src.is_contiguous() else src.contiguous()
            L.check(lib.enslam_grid_to_voxel_major(_ptr(src), _ptr(e.vm), e.vm.shape[0], _stream()), "grid_to_voxel_major")
            e.version = g._version
            n += 1
        dec = getattr(decoders, L.MLP_NAMES[k])
        cache = _pack_caches.get(dec)
        if cache is None or cache.packed is None or cache.tag != 0:
            continue
        ps = decoder_params(dec, k)
        key = _params_key(cache, ps)
        if key != cache.key:
            where = key[:2]
            if where != getattr(cache, 'where', None) or getattr(cache, 'struct', None) is None:
                _check_params(k, ps)
                cache.where, cache.struct = where, _fill_params_struct(k, ps)
            L.check(lib.enslam_pack_mlp(k, ctypes.byref(cache.struct), _ptr(cache.packed), _stream()), "enslam_pack_mlp")
            cache.key = key
            n += 1
    return n


def _scene_struct(stage, bound, coarse_bound, grids_vm, grid_dims, packed):
    """enslam_scene for a stage. grids_vm / packed: dict kind -> tensor."""
    sc = L.Scene()
    sc.bound = bound
    sc.coarse_bound = coarse_bound
    for k in range(4):
        if k in grids_vm:
            sc.grids[k].data = grids_vm[k].data_ptr()
            sc.grids[k].D, sc.grids[k].H, sc.grids[k].W = grid_dims[k]
        if k in packed:
            sc.packed[k] = packed[k].data_ptr()
    return sc


def stage_kinds(stage):
    return L.STAGE_KINDS[stage]


# ------------------------------------------------------------------------------------------------
# the differentiable render call
# ------------------------------------------------------------------------------------------------
USE_WORK_LIST = os.environ.get('ENSLAM_WORK_LIST', '1') == '1'     # process-wide default of RenderState.use_work_list


class RenderState:
    """What a render call leaves behind for its caller, per Renderer (two renderers -- a tracker's and a mapper's in one
    process, possibly on different streams -- do not see each other's):
      flags    {id(grid tensor): uint8 flags} of the 64-voxel blocks the latest call touched (parallel.allreduce_gradients
               sends only those); under hipGraph replay the buffers are rewritten in place by every replay
      work     (counter tensor, number of tiles) of the latest call's backward work list
      profile  {'decoder_bwd': [(event, event), ...]} when a caller (bench.py) asks for per-kernel timing
      use_work_list  whether this renderer's backwards walk the work list of active tiles (default) or every tile"""

    def __init__(self):
        self.flags = {}
        self.work = (None, 0)
        self.profile = {}
        # the backward walks only the 16-sample tiles whose d_raw is not all zero (per renderer; ENSLAM_WORK_LIST=0 sets the
        # process-wide default to every tile -- a diagnostic: the results are the same)
        self.use_work_list = USE_WORK_LIST

    def last_block_flags(self):
        return dict(self.flags)

    def last_active_tile_fraction(self):
        """Share of the 16-sample tiles of the most recent render call that its backward scheduled (work list of tiles
        with non-zero d_raw); None when that call kept no list.  Synchronises."""
        wcount, n = self.work
        if wcount is None or n == 0:
            return None
        return float(wcount.item()) / n


_default_state = RenderState()      # calls made without a Renderer (functional.render with a bare plan)
_latest_state = [_default_state]


def last_block_flags():
    """`RenderState.last_block_flags()` of whichever renderer rendered last in this process (single-renderer callers)."""
    return _latest_state[0].last_block_flags()


class VoxelMajorGrid:
    """A feature grid kept in the kernels' own layout across iterations (see mapper.MaskedGridOptimizer):
    `vm` float32 [V,32] values, `grad_vm` float32 [V,32] gradient accumulator that render backwards ADD into and
    the optimiser consumes and clears.  Passing one of these in the `c` dict of Renderer.render_batch_ray skips the
    per-call layout conversion, block marking, accumulator clearing and transposed-back gradient.  `anchor` is the
    tensor that ties the object into autograd (its own gradient is always None)."""

    def __init__(self, dims, vm, grad_vm):
        self.dims = tuple(int(d) for d in dims)
        V = self.dims[0] * self.dims[1] * self.dims[2]
        for t, name in ((vm, "vm"), (grad_vm, "grad_vm")):
            _require_hip(t, name)
            if tuple(t.shape) != (V, 32) or t.dtype != torch.float32 or not t.is_contiguous():
                raise L.EnslamError(f"VoxelMajorGrid.{name}: expected contiguous float32 [{V},32], got {tuple(t.shape)} {t.dtype}")
        self.vm, self.grad_vm = vm, grad_vm
        self.anchor = torch.zeros(1, dtype=torch.float32, device=vm.device, requires_grad=True)
        self.has_grad = False           # set by a backward that added into grad_vm

    @property
    def shape(self):
        return (1, 32) + self.dims

    @property
    def device(self):
        return self.vm.device

    @property
    def requires_grad(self):
        return self.anchor.requires_grad


class RenderPlan:
    """Static description of one render_batch_ray call (everything that is not a differentiable tensor)."""

    def __init__(self, stage, bound, coarse_bound, n_lin, n_surf, lindisp, t_lin, t_surf, kinds, decoders,
                 depth_max=None):
        self.stage = stage
        self.depth_max = depth_max              # float32 [2] {max, fl32(max*1.2)} of the WHOLE batch, or None
        self.bound6 = bound6(bound)
        self.coarse_bound6 = bound6(coarse_bound)
        self.n_lin, self.n_surf, self.lindisp = n_lin, n_surf, int(bool(lindisp))
        self.t_lin, self.t_surf = t_lin, t_surf
        self.kinds = kinds                      # decoder / grid kinds used, ascending
        self.decoders = decoders                # dict kind -> module
        self.n_params = {k: (12 if k == L.MLP_COARSE else 23) for k in kinds}
        self.vm = {}                            # kind -> VoxelMajorGrid for grids passed in the device layout
        self.loss = None                        # (gt_depth [N] f32, gt_color [N,3] f32 | None, w_color): fused mapper loss
        self.state = _default_state             # the calling Renderer's RenderState
        # hierarchical sampling's second pass (Renderer.py:182-197): sample distances given by the caller instead of the
        # sampler -- float64 [N, S] with S a multiple of 16 (<= 64), of which the first s_valid per ray are real samples
        # (the rest pad the last tile: evaluated, but left out of the compositing and given zero gradient)
        self.z_given = None
        self.s_valid = None


class _Accumulators:
    """The buffers a render backward adds into: voxel-major grid gradients (only the touched blocks are ever cleared,
    read or transposed back) and one flat buffer of packed-layout decoder gradients and ray gradients.  Laid out in
    the forward, because the launch that prepares the forward's inputs clears them as well."""

    def __init__(self, plan, dims, needs, N, dev, lib, native=(), grid_ids=None):
        nk = len(plan.kinds)
        self.need_rays = bool(needs[1] or needs[2])
        self.need_grid = {k: bool(needs[5 + i]) for i, k in enumerate(plan.kinds)}
        off, self.need_par = 5 + nk, {}
        for k in plan.kinds:
            n = plan.n_params[k]
            self.need_par[k] = any(needs[off:off + n])
            off += n
        # Gradients of grids that arrive in the kernels' own layout (channels_last_3d tensors, `native`): the buffer the backward
        # adds into IS the tensor autograd receives.  Eagerly it is a slice of the flat buffer below (fresh and cleared as a whole
        # per call); under hipGraph capture it is the same memory at every replay and only the blocks the previous replay
        # touched are cleared (nat_persist: kind -> (gradient buffer [V*32], prev flags); the flags move there in the finish
        # launch).  A second render of the same grid inside one captured step is not persistent (see _RenderFn.backward).
        self.native = {k: (k in native and self.need_grid[k]) for k in plan.kinds}
        self.nat_persist, self.nat_again = {}, {}
        persist_ok = _capturing() and _capture['init_zero'] is not None
        sizes = []
        for k in plan.kinds:
            D, H, W = dims[k]
            sizes.append(D * H * W * 32 if (self.need_grid[k] and k not in plan.vm and not self.native[k]) else 0)
        for k in plan.kinds:
            sizes.append(_lib_size('enslam_packed_grad_floats', k) if self.need_par[k] else 0)
        sizes.append(6 * N if self.need_rays else 0)
        pers = []
        for i, k in enumerate(plan.kinds):
            D, H, W = dims[k]
            n = D * H * W * 32 if self.native[k] else 0
            if n and persist_ok:
                if grid_ids[i] in _capture['persist']:
                    self.nat_again[k] = grid_ids[i]
                else:
                    pers.append((i, k, n))
                    n = 0
            sizes.append(n)
        offs = [0]
        for n in sizes:
            offs.append(offs[-1] + n)
        self.sizes, self.offs = sizes, offs
        self.n_grid = offs[nk]
        self.n_flat = offs[-1] - self.n_grid
        self.gbuf = torch.empty(max(self.n_grid, 1), dtype=torch.float32, device=dev)
        # flat part + 16 bytes the same launch clears: the work-list counter (int32) and the fused loss (float64) of a
        # captured training step live here instead of in a zero-filled arena
        self.tail = (self.n_flat + 1) & ~1
        self.n_zero = self.tail + 4
        self.zbuf = torch.empty(self.n_zero, dtype=torch.float32, device=dev)
        self.clean = False          # set by the launch that cleared them; a backward consumes it
        self.pv_flat = None
        if pers:
            nblk = [(n // 32 + 63) // 64 for _i, _k, n in pers]
            self.pv_flat = torch.empty(sum(nblk), dtype=torch.uint8, device=dev)
            _capture['init_zero'].append(self.pv_flat.untyped_storage())
            for (i, k, n), pv in zip(pers, self.pv_flat.split(nblk)):
                g = torch.empty(n, dtype=torch.float32, device=dev)
                _capture['init_zero'].append(g.untyped_storage())
                _capture['persist'][grid_ids[i]] = (g.data_ptr(), pv)
                _persist_register(g, pv)
                self.nat_persist[k] = (g, pv)

    def native_grad(self, plan, k):
        """flat [V*32] gradient buffer of native grid kind k"""
        if k in self.nat_persist:
            return self.nat_persist[k][0]
        i = plan.kinds.index(k)
        j = 2 * len(plan.kinds) + 1 + i
        o = self.offs[j] - self.n_grid
        return self.zbuf[o:o + self.sizes[j]]

    def counter(self):
        return self.zbuf[self.tail:self.tail + 1].view(torch.int32)

    def loss_slot(self):
        return self.zbuf[self.tail + 2:self.tail + 4].view(torch.float64)

    def zero_args(self, plan, flags):
        """(n, dsts, n_voxels, need flags) of the grid accumulators for enslam_zero_blocks / enslam_step_prepare."""
        zl = [(i, k) for i, k in enumerate(plan.kinds) if self.need_grid[k] and k not in plan.vm and not self.native[k]]
        n = len(zl) + len(self.nat_persist)
        dsts, vs, nd = (ctypes.c_void_p * max(n, 1))(), (ctypes.c_int64 * max(n, 1))(), (ctypes.c_void_p * max(n, 1))()
        for j, (i, k) in enumerate(zl):
            dsts[j], vs[j], nd[j] = self.gbuf.data_ptr() + 4 * self.offs[i], self.sizes[i] // 32, flags[i].data_ptr()
        for j, (g, pv) in enumerate(self.nat_persist.values()):      # persistent native gradients: the blocks touched one replay ago
            dsts[len(zl) + j], vs[len(zl) + j], nd[len(zl) + j] = g.data_ptr(), g.numel() // 32, pv.data_ptr()
        return n, dsts, vs, nd


class _RenderFn(torch.autograd.Function):
    """inputs: plan, rays_o, rays_d, gt_depth|None, t_rand|None, then for each kind in plan.kinds: grid,
    then for each kind: its parameters.  Outputs depth f64 [N], var f64 [N], rgb f32 [N,3]; with plan.loss the
    fused mapper loss (f64 scalar) comes first and is the only differentiable output."""

    @staticmethod
    def forward(ctx, plan, rays_o, rays_d, gt_depth, t_rand, *tensors):
        lib = L.lib()
        ctx.set_materialize_grads(False)          # unused outputs (the variance) arrive as None, not as a zero fill
        nk = len(plan.kinds)
        grids = tensors[:nk]
        N = rays_o.shape[0]
        dev = rays_o.device
        S = plan.n_lin + (plan.n_surf if gt_depth is not None else 0)
        st = _stream()
        ro, rd = _f32c(rays_o), _f32c(rays_d)
        gd = _f32c(gt_depth).reshape(-1) if gt_depth is not None else None
        SV = None                                   # real samples per ray when the last tile is padded
        if plan.z_given is not None:
            z = plan.z_given.detach().to(torch.float64).contiguous()
            S = int(z.shape[1])
            if tuple(z.shape) != (N, S) or S % 16 != 0 or S > 64 or plan.loss is not None:
                raise L.EnslamError(f"given sample distances must be float64 [N, 16k <= 64] without a fused loss, got {tuple(z.shape)}")
            if plan.s_valid is not None and plan.s_valid < S:
                SV = int(plan.s_valid)
        else:
            z = torch.empty((N, S), dtype=torch.float64, device=dev)
        scratch = plan.depth_max if plan.depth_max is not None else torch.empty(2, dtype=torch.float32, device=dev)
        # blocks of 64 voxels this batch touches, per grid (one zeroed byte buffer for all grids).  Grids that
        # arrive in the device layout (plan.vm) need none of this.
        vmg = plan.vm
        dims = {k: (vmg[k].dims if k in vmg else tuple(g.shape[2:])) for k, g in zip(plan.kinds, grids)}
        # grids without gradient (tracker, render_img, Mesher): one full conversion per grid version, cached -- the map
        # does not change between the camera iterations of a frame, so nothing is marked or converted per call
        # grids in the kernels' own layout (channels_last_3d tensors): read where they lie, never converted
        native = {k for i, k in enumerate(plan.kinds) if k not in vmg and is_native_grid(grids[i])}
        static = [(i, k) for i, k in enumerate(plan.kinds) if k not in vmg and k not in native and not ctx.needs_input_grad[5 + i]]
        dense = [(i, k) for i, k in enumerate(plan.kinds) if k not in vmg and ctx.needs_input_grad[5 + i]]
        nblk = [(dims[k][0] * dims[k][1] * dims[k][2] + 63) // 64 for _, k in dense]
        # A captured training step (fused render + loss: its backward always follows) needs no zero-fill node at all: the
        # block flags are cleared by the finish launch that consumes them (enslam_step_finish_rays_prev), the packed
        # decoders' padding stays zero, the conversion runs without a validity bitmap and the two accumulating scalars sit
        # in the flat buffer the prepare launch clears.  Everywhere else: one zero-filled arena per call.
        cap = bool(_capturing() and _capture['init_zero'] is not None and plan.loss is not None and plan.z_given is None
                   and any(ctx.needs_input_grad[5:5 + nk]))
        arena = _ZeroArena(dev, 2 * sum(nblk) + 4 * sum(_lib_size('enslam_packed_floats', k) for k in plan.kinds) + 256 + 32, persistent=cap)
        flags = [None] * nk
        grids_vm, packed = {k: vmg[k].vm for k in vmg}, {}
        for i, k in enumerate(plan.kinds):
            if k in native:
                _check_grid(grids[i])
                grids_vm[k] = grids[i].detach()
        state = plan.state
        _latest_state[0] = state
        state.flags = {}
        accum = None
        if any(ctx.needs_input_grad):
            accum = _Accumulators(plan, dims, ctx.needs_input_grad, N, dev, lib, native, [id(g) for g in grids])
        msc, fptr = None, None
        flag_move = None                # (flags, prev flags) of the persistent native gradients: one contiguous range each
        if dense:                       # the sampler marks the blocks of the samples it places
            # the flags of persistent native gradients sit together, in the order of their `prev` flags (the finish launch moves
            # them there as one range)
            order = [j for j, (_i, k) in enumerate(dense) if k in accum.nat_persist] + \
                    [j for j, (_i, k) in enumerate(dense) if k not in accum.nat_persist]
            flag_buf = arena.take(sum(nblk), torch.uint8)
            fptr = (ctypes.c_void_p * 4)()
            msc = L.Scene()
            msc.bound, msc.coarse_bound = plan.bound6, plan.coarse_bound6
            for j, fl in zip(order, flag_buf.split([nblk[j] for j in order])):
                i, k = dense[j]
                flags[i] = fl
                fptr[k] = fl.data_ptr()
                msc.grids[k].D, msc.grids[k].H, msc.grids[k].W = dims[k]
                state.flags[id(grids[i])] = fl
            if accum.pv_flat is not None:
                flag_move = (flag_buf[:accum.pv_flat.numel()], accum.pv_flat)
        conv = [(i, k) for i, k in dense if k not in native]
        merged = plan.z_given is None and not conv        # nothing to convert: the sampler and the prepare roles in one launch
        if merged:
            pass
        elif plan.z_given is None:
            L.check(lib.enslam_sample_rays(N, plan.n_lin, plan.n_surf, _ptr(ro), _ptr(rd), _ptr(gd), plan.bound6,
                                           _ptr(plan.t_lin), _ptr(plan.t_surf), plan.lindisp, _ptr(t_rand),
                                           _ptr(scratch), int(plan.depth_max is not None), _ptr(z), L.STAGE[plan.stage],
                                           ctypes.byref(msc) if msc is not None else None, fptr, st),
                    "enslam_sample_rays")
        elif msc is not None:                       # the samples are given: block marking as a launch of its own
            L.check(lib.enslam_mark_blocks(L.STAGE[plan.stage], N, S, _ptr(ro), _ptr(rd), _ptr(z), ctypes.byref(msc), fptr, st),
                    "enslam_mark_blocks")
        if static:
            for (i, k), vm in zip(static, _grid_cache.get_many([grids[i] for i, _ in static])):
                grids_vm[k] = vm
        conv_args = None
        if conv:
            conv_grids = [grids[i] for i, _ in conv]
            vms, conv_args = _grid_cache.get_many_sparse(conv_grids, [flags[i] for i, _ in conv], arena, defer=True, fresh=cap)
            for (i, k), vm in zip(conv, vms):
                grids_vm[k] = vm
        po, items = nk, []
        for k in plan.kinds:
            items.append((plan.decoders[k], k, tensors[po:po + plan.n_params[k]]))
            po += plan.n_params[k]
        pks, pack_args, pack_commit = packed_decoders(items, arena, defer=True)
        for k, pk in zip(plan.kinds, pks):
            packed[k] = pk
        # ONE launch: pack the stale decoders, convert the touched blocks, clear the backward's accumulators
        nd_, kinds_, structs_, ptrs_ = pack_args if pack_args is not None else (0, None, None, None)
        nc_, srcs_, dsts_, vs_, needs_, valids_, keep_ = conv_args if conv_args is not None else (0, None, None, None, None, None, None)
        nz_, zd_, zv_, zn_ = accum.zero_args(plan, flags) if accum is not None else (0, None, None, None)
        if merged:
            L.check(lib.enslam_sample_prepare(N, plan.n_lin, plan.n_surf, _ptr(ro), _ptr(rd), _ptr(gd), plan.bound6,
                                              _ptr(plan.t_lin), _ptr(plan.t_surf), plan.lindisp, _ptr(t_rand),
                                              _ptr(scratch), int(plan.depth_max is not None), _ptr(z), L.STAGE[plan.stage],
                                              ctypes.byref(msc) if msc is not None else None, fptr, 64, None,
                                              nd_, kinds_, structs_, ptrs_, nz_, zd_, zv_, zn_,
                                              _ptr(accum.zbuf) if accum is not None else None,
                                              accum.n_zero if accum is not None else 0, st), "enslam_sample_prepare")
            if accum is not None:
                accum.clean = True
        elif nd_ or nc_ or accum is not None:
            L.check(lib.enslam_step_prepare(nd_, kinds_, structs_, ptrs_, nc_, srcs_, dsts_, vs_, needs_, valids_, nz_, zd_, zv_, zn_,
                                            _ptr(accum.zbuf) if accum is not None else None,
                                            accum.n_zero if accum is not None else 0, st), "enslam_step_prepare")
            if accum is not None:
                accum.clean = True
        pack_commit()
        del keep_
        sc = _scene_struct(plan.stage, plan.bound6, plan.coarse_bound6, grids_vm, dims, packed)
        depth = torch.empty(N, dtype=torch.float64, device=dev)
        var = torch.empty(N, dtype=torch.float64, device=dev)
        rgb = torch.empty((N, 3), dtype=torch.float32, device=dev)
        raw = torch.empty((N * S, 4), dtype=torch.float32, device=dev)
        # a backward will follow: let the forward park the backward's operands (else the backward recomputes them)
        act = None
        # no decoder parameter wants a gradient (tracker; mapper stages with fixed decoders): the light workspace
        act_light = int(not any(ctx.needs_input_grad[5 + nk:]))
        if any(ctx.needs_input_grad):
            n_act = _lib_size('enslam_activation_floats', L.STAGE[plan.stage], N, S, act_light)
            if 0 < n_act * 4 <= ACT_WORKSPACE_LIMIT_BYTES and max(d[0] * d[1] * d[2] for d in dims.values()) < (1 << 29):
                act = torch.empty(n_act, dtype=torch.float32, device=dev)
        loss = None
        # work list of the backward (tiles with non-zero d_raw): filled by whichever kernel produces d_raw; the counter
        # comes zeroed out of this call's arena
        work = wcount = None
        if act is not None and state.use_work_list and any(ctx.needs_input_grad) and SV is None:
            work = torch.empty(N * (S // 16), dtype=torch.int32, device=dev)
            wcount = accum.counter() if accum is not None else arena.take(1, torch.int32)    # (cleared by the prepare launch)
        if plan.loss is None:
            L.check(lib.enslam_render_fwd(L.STAGE[plan.stage], N, S, _ptr(ro), _ptr(rd), _ptr(z), ctypes.byref(sc),
                                          _ptr(depth), _ptr(var), _ptr(rgb), _ptr(raw), _ptr(act), act_light, st),
                    "enslam_render_fwd")
        else:
            lgd, lgc, lw = plan.loss[:3]
            loss = accum.loss_slot() if accum is not None else arena.take(1, torch.float64)
            # the compositing launch also leaves d(loss)/d(raw) for a unit loss gradient: the backward starts at the decoders
            d_raw_unit = torch.empty((N * S, 4), dtype=torch.float32, device=dev) if any(ctx.needs_input_grad) else None
            if len(plan.loss) > 3:              # the tracker's loss (Tracker.py:176-195): (gd, gc, w, inside mask | None, handle_dynamic, 'tracker')
                linside, ldyn = plan.loss[3], plan.loss[4]
                tmp = torch.empty(N, dtype=torch.float64, device=dev)
                L.check(lib.enslam_render_tracker_loss_fwd(L.STAGE[plan.stage], N, S, _ptr(ro), _ptr(rd), _ptr(z), ctypes.byref(sc),
                                                           _ptr(depth), _ptr(var), _ptr(rgb), _ptr(raw), _ptr(act), act_light, _ptr(lgd),
                                                           _ptr(lgc), ctypes.c_float(lw), _ptr(linside), int(bool(ldyn)), _ptr(tmp),
                                                           _ptr(loss), _ptr(d_raw_unit),
                                                           _ptr(work) if d_raw_unit is not None else None,
                                                           _ptr(wcount) if d_raw_unit is not None else None, st),
                        "enslam_render_tracker_loss_fwd")
            else:
                L.check(lib.enslam_render_loss_fwd(L.STAGE[plan.stage], N, S, _ptr(ro), _ptr(rd), _ptr(z), ctypes.byref(sc),
                                                   _ptr(depth), _ptr(var), _ptr(rgb), _ptr(raw), _ptr(act), act_light, _ptr(lgd),
                                                   _ptr(lgc), ctypes.c_float(lw), _ptr(loss), _ptr(d_raw_unit),
                                                   _ptr(work) if d_raw_unit is not None else None,
                                                   _ptr(wcount) if d_raw_unit is not None else None, st),
                        "enslam_render_loss_fwd")
        ctx.sv = None
        if SV is not None:
            # compositing over the real samples only (the kernels above composited the padded rays): contiguous [N, SV] views
            raw_v = raw.view(N, S, 4)[:, :SV].contiguous()
            z_v = z[:, :SV].contiguous()
            L.check(lib.enslam_composite_fwd(N, SV, _ptr(raw_v), _ptr(z_v), _ptr(depth), _ptr(var), _ptr(rgb), None, st),
                    "enslam_composite_fwd")
            ctx.sv = (SV, raw_v, z_v)
        ctx.plan, ctx.S, ctx.dims, ctx.act_light, ctx.accum = plan, S, dims, act_light, accum
        ctx.cap_arena = cap
        ctx.flag_move = flag_move
        if accum is not None:
            for i, k in enumerate(plan.kinds):
                if k in accum.nat_persist:
                    _capture['persist_need'][id(grids[i])] = flags[i]
                elif k in accum.nat_again:
                    # a second render of this grid inside one captured step: its gradient is a fresh buffer that AccumulateGrad adds
                    # into the first call's persistent one, so the blocks it touches must reach that buffer's `prev` flags whatever the
                    # order of the two backwards -- joined to the first call's flags here (moved to `prev` by its finish launch if
                    # that is still to come) and to `prev` itself after this call's backward
                    need_first = _capture['persist_need'].get(id(grids[i]))
                    if need_first is not None:
                        torch.maximum(need_first, flags[i], out=need_first)
        ctx.keep = (ro, rd, z, raw, depth, grids_vm, packed, act, flags)
        ctx.live_guard = _live_grid_guard(grids) if any(ctx.needs_input_grad) and not _cap_tag() else []
        ctx.rgb = rgb if plan.loss is not None else None
        ctx.d_raw_unit = d_raw_unit if plan.loss is not None else None
        ctx.work, ctx.wcount = work, wcount
        state.work = (wcount, N * (S // 16))
        ctx.work_filled = plan.loss is not None and work is not None and d_raw_unit is not None      # (by the forward)
        ctx.grid_shapes = [tuple(g.shape) for g in grids]
        ctx.grid_ids = [id(g) for g in grids]
        ctx.param_like = tensors[nk:]
        if loss is not None:
            ctx.mark_non_differentiable(depth, var, rgb)
            return loss[0], depth, var, rgb
        return depth, var, rgb

    @staticmethod
    def backward(ctx, *gouts):
        lib = L.lib()
        plan, S = ctx.plan, ctx.S
        g_loss = None
        if plan.loss is not None:
            g_loss, g_depth, g_var, g_rgb = gouts[0], None, None, None
        else:
            g_depth, g_var, g_rgb = gouts
        ro, rd, z, raw, depth, grids_vm, packed, act, flags = ctx.keep
        _check_live_grids(ctx.live_guard)
        N, dev, st = ro.shape[0], ro.device, _stream()
        nk = len(plan.kinds)
        needs = ctx.needs_input_grad            # (plan, ro, rd, gd, t_rand, grids..., params...)
        accum = ctx.accum
        need_rays, need_grid, need_par = accum.need_rays, accum.need_grid, accum.need_par

        def prep(g, dtype, shape):
            if g is None:
                return None
            g = g.detach()
            if g.dtype is not dtype:
                g = g.to(dtype)
            if tuple(g.shape) != shape:
                g = g.expand(shape)
            return g if g.is_contiguous() else g.contiguous()

        gD, gV, gC = prep(g_depth, torch.float64, (N,)), prep(g_var, torch.float64, (N,)), prep(g_rgb, torch.float32, (N, 3))
        gL = prep(g_loss, torch.float64, (1,))
        if gD is None and gV is None and gC is None and gL is None:
            return (None,) * len(needs)
        sc = _scene_struct(plan.stage, plan.bound6, plan.coarse_bound6, grids_vm, ctx.dims, packed)
        gg = (L.Grid * 4)()
        gpk = (ctypes.c_void_p * 4)()
        # accumulators: laid out and cleared by the forward's prepare launch (cleared again here on a repeated backward)
        vmg = plan.vm               # grids in the device layout accumulate into their own grad_vm (kept clear by the optimiser)
        sizes, offs, n_grid, n_flat, gbuf, zbuf = accum.sizes, accum.offs, accum.n_grid, accum.n_flat, accum.gbuf, accum.zbuf
        for k in plan.kinds:
            D, H, W = ctx.dims[k]
            gg[k].D, gg[k].H, gg[k].W = D, H, W
            if need_grid[k] and k in vmg:
                gg[k].data = vmg[k].grad_vm.data_ptr()
                vmg[k].has_grad = True
        gbase = gbuf.data_ptr()
        g_grids_vm, g_packed = {}, {}
        for i, k in enumerate(plan.kinds):
            if need_grid[k] and k not in vmg:
                g_grids_vm[k] = gbase + 4 * offs[i]
                gg[k].data = g_grids_vm[k]
        nat = accum.native
        if not accum.clean:
            # a repeated backward of this call (retain_graph): the flat buffer of the first one backs tensors it returned (ray
            # gradients, native grid gradients) -- this one adds into a fresh, zero-filled buffer
            if accum.nat_persist:
                raise L.EnslamError("a second backward through the same render call inside one captured step is not supported for "
                                    "channels_last_3d feature grids (their gradient buffer is the graph's own)")
            zbuf = accum.zbuf = torch.zeros(accum.n_zero, dtype=torch.float32, device=dev)
            n, dsts, vs, need_ptrs = accum.zero_args(plan, flags)
            if n:
                L.check(lib.enslam_zero_blocks(n, dsts, vs, need_ptrs, None, 0, st), "enslam_zero_blocks")
        accum.clean = False
        zbase = zbuf.data_ptr() - 4 * n_grid
        nat_buf = {}
        for k in plan.kinds:
            if nat[k]:
                nat_buf[k] = accum.native_grad(plan, k)
                gg[k].data = nat_buf[k].data_ptr()
        # decoder-parameter gradients leave the backward kernel as per-workgroup partial images (summed by the finish launch)
        # instead of 4.4 M float atomics at its tail; ENSLAM_DW_PARTIALS=0 restores the atomics (A/B aid)
        gpart, part_keep = (ctypes.c_void_p * 4)(), {}
        for i, k in enumerate(plan.kinds):
            if need_par[k]:
                g_packed[k] = zbase + 4 * offs[nk + i]
                gpk[k] = g_packed[k]
                if USE_DW_PARTIALS:
                    part_keep[k] = torch.empty(_lib_size('enslam_bwd_partial_floats', k), dtype=torch.float32, device=dev)
                    gpart[k] = part_keep[k].data_ptr()
        g_ro = g_rd = None
        p_ro = p_rd = None
        if need_rays:
            r0 = offs[2 * nk] - n_grid
            g_ro = zbuf[r0:r0 + 3 * N].view(N, 3)
            g_rd = zbuf[r0 + 3 * N:r0 + 6 * N].view(N, 3)
            p_ro, p_rd = _ptr(g_ro), _ptr(g_rd)
        d_scale = None
        work, wcount = ctx.work, ctx.wcount
        if work is not None and not (gL is not None and ctx.d_raw_unit is not None):
            if ctx.work_filled:                             # a repeated backward appends again: start from an empty list
                wcount.zero_()
            ctx.work_filled = True
        if gL is not None and ctx.d_raw_unit is not None:
            d_raw, d_scale = ctx.d_raw_unit, gL             # unit gradients from the forward, scaled inside the decoder backward
        elif gL is not None:
            d_raw = torch.empty((N * S, 4), dtype=torch.float32, device=dev)
            if len(plan.loss) > 3:
                raise L.EnslamError("the tracker's fused loss keeps its unit gradients from the forward; none were kept")
            lgd, lgc, lw = plan.loss
            L.check(lib.enslam_composite_loss_bwd(N, S, _ptr(raw), _ptr(z), _ptr(depth), _ptr(ctx.rgb), _ptr(lgd), _ptr(lgc),
                                                  ctypes.c_float(lw), _ptr(gL), _ptr(d_raw), _ptr(work), _ptr(wcount), st),
                    "enslam_composite_loss_bwd")
        elif ctx.sv is not None:                            # padded last tile: gradient of the real samples, zeros for the pad
            SV, raw_v, z_v = ctx.sv
            d_raw_v = torch.empty((N, SV, 4), dtype=torch.float32, device=dev)
            L.check(lib.enslam_composite_bwd(N, SV, _ptr(raw_v), _ptr(z_v), _ptr(depth), _ptr(gD), _ptr(gV), _ptr(gC),
                                             _ptr(d_raw_v), st), "enslam_composite_bwd")
            d_raw = torch.zeros((N, S, 4), dtype=torch.float32, device=dev)
            d_raw[:, :SV] = d_raw_v
            d_raw = d_raw.view(N * S, 4)
        else:
            d_raw = torch.empty((N * S, 4), dtype=torch.float32, device=dev)
            L.check(lib.enslam_composite_bwd_list(N, S, _ptr(raw), _ptr(z), _ptr(depth), _ptr(gD), _ptr(gV), _ptr(gC),
                                                  _ptr(d_raw), _ptr(work), _ptr(wcount), st), "enslam_composite_bwd")
        # Ray gradients of the saved-activation path: handed to the ray-gradient role of the finish launch through dgw when
        # that launch exists anyway (grid gradients to transpose back, decoder gradients to unpack: in-kernel ray gradients
        # cost the mapper step's backward 15 us to save 11 in the finish launch), else computed by the decoder kernel itself at
        # the end of each round -- a tracker iteration (fixed map and decoders) then has no finish launch at all: 104 -> 100 us.
        # ENSLAM_INLINE_RAY_GRAD = 1 / 0 forces one or the other.
        finish_needed = any((need_grid[k] and k not in plan.vm and not nat[k]) or need_par[k] for k in plan.kinds) or bool(accum.nat_persist)
        inline_rays = (not finish_needed) if INLINE_RAY_GRAD is None else INLINE_RAY_GRAD
        dgw = None
        # ENSLAM_DEFER_SCATTER=1 / 2 (opt-in, csrc/grid_scatter.hip): the decoder kernels leave dC in the same hand-off and a launch of its
        # own scatters it, first summing in LDS what neighbouring rays add to the same voxel rows -- always / when a decoder WITHOUT
        # parameter gradients has a grid gradient (the reference mapper's fixed occupancy decoders).  Same rule here as in the library.
        defer = False
        if DEFER_SCATTER and act is not None and plan.stage != 'coarse':
            any_grid = any(need_grid[k] for k in plan.kinds)
            light_grid = any(need_grid[k] and not need_par[k] for k in plan.kinds)
            defer = any_grid if DEFER_SCATTER == 1 else light_grid
        if act is not None and ((need_rays and not inline_rays) or defer):
            dgw = torch.empty(_lib_size('enslam_grid_handoff_floats', L.STAGE[plan.stage], N, S), dtype=torch.float32, device=dev)
        ev = plan.state.profile.get('decoder_bwd')
        if ev is not None:                      # bench.py: HIP events around the dominant kernel, on this stream
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        L.check(lib.enslam_decoder_bwd_partials(L.STAGE[plan.stage], N, S, _ptr(ro), _ptr(rd), _ptr(z), ctypes.byref(sc),
                                                _ptr(d_raw), _ptr(d_scale), _ptr(act), ctx.act_light, _ptr(dgw), gg, gpk, gpart, p_ro, p_rd,
                                                _ptr(work), _ptr(wcount), st), "enslam_decoder_bwd")
        if ev is not None:
            e1.record()
            ev.append((e0, e1))
        # saved-activation path: the ray gradients (corner re-gather from the hand-off in dgw) ride in the finish launch
        ray_pending = dgw is not None and need_rays and plan.stage != 'coarse'
        out = [None, g_ro if needs[1] else None, g_rd if needs[2] else None, None, None]
        # ONE launch: grid gradients back to the callers' [1,32,D,H,W] layout + decoder gradients unpacked into views of
        # one flat buffer shaped like the parameters
        conv = [(i, k) for i, k in enumerate(plan.kinds) if need_grid[k] and k not in vmg and not nat[k]]
        grid_out = {}
        for i, k in enumerate(plan.kinds):
            if nat[k]:                                      # (the buffer the backward kernel has just added into)
                grid_out[k] = _native_grad_view(nat_buf[k], ctx.dims[k])
                if k in accum.nat_persist:
                    plan.state.flags[ctx.grid_ids[i]] = accum.nat_persist[k][1]     # readers use `prev` from the finish launch on
        del nat_buf
        nc = len(conv)
        srcs, dsts, vs = (ctypes.c_void_p * max(nc, 1))(), (ctypes.c_void_p * max(nc, 1))(), (ctypes.c_int64 * max(nc, 1))()
        need_ptrs = (ctypes.c_void_p * max(nc, 1))()
        # Under hipGraph capture the dense gradient of a grid is the same memory at every replay: the finish launch then only
        # rewrites the blocks touched now or one replay earlier (enslam_step_finish_rays_prev) instead of zero-filling the
        # ~85 % of the tensor no ray came near.  The buffers start zeroed by end_capture(); only their STORAGES are kept
        # there (a second reference to the tensor itself would make AccumulateGrad clone the 16 MB instead of adopting it).
        persistent = _capturing() and _capture['init_zero'] is not None and nc > 0
        # A second backward into the same grid inside one captured step (AccumulateGrad adds its gradient into the first
        # one's persistent buffer) must not be persistent itself: it returns a fresh, fully written gradient, and the blocks
        # it touched join the first buffer's flags (a captured elementwise max below), so the next replay clears them there.
        again = [ctx.grid_ids[i] for i, _k in conv if persistent and ctx.grid_ids[i] in _capture['persist']]
        if again:
            persistent = False
        prev_ptrs = (ctypes.c_void_p * max(nc, 1))() if persistent else None
        prev_keep = []
        for j, (i, k) in enumerate(conv):
            g = torch.empty(ctx.grid_shapes[i], dtype=torch.float32, device=dev)
            grid_out[k] = g
            srcs[j], dsts[j], vs[j], need_ptrs[j] = g_grids_vm[k], g.data_ptr(), sizes[i] // 32, flags[i].data_ptr()
            if persistent:
                pv = torch.empty(flags[i].numel(), dtype=torch.uint8, device=dev)
                prev_ptrs[j] = pv.data_ptr()
                prev_keep.append(pv)
                plan.state.flags[ctx.grid_ids[i]] = pv      # the launch moves the flags there (last_block_flags)
                _capture['init_zero'] += [g.untyped_storage(), pv.untyped_storage()]
                _capture['persist'][ctx.grid_ids[i]] = (g.data_ptr(), pv)
                _persist_register(g, pv)
        for k in plan.kinds:
            out.append(grid_out.get(k))
        kinds_p = [k for k in plan.kinds if need_par[k]]
        views_by_kind = {}
        npk = len(kinds_p)
        kind_arr, pk_arr, structs = (ctypes.c_int32 * max(npk, 1))(), (ctypes.c_void_p * max(npk, 1))(), (L.MlpParams * max(npk, 1))()
        part_arr = (ctypes.c_void_p * max(npk, 1))()
        if kinds_p:
            # the gradients of all decoder parameters are views of ONE fresh flat buffer, shaped like the parameters by one
            # C++ call (69 x split + view in Python cost 0.19 ms per step); the pointer structs come from the flat base and
            # the parameters' (fixed) sizes
            like, po = [], nk
            like_by_kind = {}
            for k in plan.kinds:
                if need_par[k]:
                    like_by_kind[k] = ctx.param_like[po - nk:po - nk + plan.n_params[k]]
                    like += like_by_kind[k]
                po += plan.n_params[k]
            total = sum(t.numel() for t in like)
            pflat = torch.empty(total, dtype=torch.float32, device=dev)
            views = torch._C._nn.unflatten_dense_tensors(pflat, like)
            base, vo = pflat.data_ptr(), 0
            for j, k in enumerate(kinds_p):
                n = plan.n_params[k]
                views_by_kind[k] = list(views[vo:vo + n])
                vo += n
                kind_arr[j], pk_arr[j] = k, g_packed[k]
                part_arr[j] = gpart[k]
                structs[j], base = _flat_params_struct(k, like_by_kind[k], base)
        mv = ctx.flag_move
        if nc or npk or ray_pending or mv is not None:
            L.check(lib.enslam_step_finish_native(nc, srcs, dsts, vs, need_ptrs, prev_ptrs, npk, kind_arr, pk_arr, part_arr, structs,
                                                  L.STAGE[plan.stage], N if ray_pending else 0, S, _ptr(ro), _ptr(rd), _ptr(z),
                                                  ctypes.byref(sc), _ptr(dgw) if ray_pending else None, p_ro, p_rd, _ptr(work),
                                                  _ptr(wcount), _ptr(mv[0]) if mv is not None else None,
                                                  _ptr(mv[1]) if mv is not None else None, mv[0].numel() if mv is not None else 0, st),
                    "enslam_step_finish")
        for i, k in enumerate(plan.kinds):
            gid = ctx.grid_ids[i]
            if (need_grid[k] and k not in vmg and not nat[k] and gid in again) or k in accum.nat_again:
                # (captured: runs at every replay, after the finish launch)
                pv_first = _capture['persist'][gid][1] if _capture['persist'] is not None and gid in _capture['persist'] else None
                if pv_first is not None:
                    torch.maximum(pv_first, flags[i], out=pv_first)
                    if ctx.cap_arena:
                        flags[i].zero_()                    # no fill node re-zeroes a captured step's arena
        for k in plan.kinds:
            out += views_by_kind.get(k, [None] * plan.n_params[k])
        return tuple(out)       # (the saved buffers go with the graph; kept so that retain_graph backwards work)


# The forward keeps the backward's operands (1.3 KB per sample and decoder: 172 MB at 1000 rays x 48, colour
# stage) when their total stays under this limit; above it the backward recomputes them (slower, no extra memory).
ACT_WORKSPACE_LIMIT_BYTES = 8 << 30

INLINE_RAY_GRAD = {'1': True, '0': False}.get(os.environ.get('ENSLAM_INLINE_RAY_GRAD', ''), None)     # None: decided per call
DEFER_SCATTER = {'1': 1, '2': 2}.get(os.environ.get('ENSLAM_DEFER_SCATTER', ''), 0)    # feature-gradient scatter as its own launch (csrc/grid_scatter.hip): off (default) / always / by policy
# weight gradients as per-workgroup partial images summed by the finish launch instead of float atomics at the backward's tail:
# backward 138 -> 132 us, finish launch 22 -> 28 us (17.6 MB more to read), step unchanged -- off by default (round 3)
USE_DW_PARTIALS = os.environ.get('ENSLAM_DW_PARTIALS', '0') == '1'


def last_active_tile_fraction():
    """`RenderState.last_active_tile_fraction()` of whichever renderer rendered last in this process."""
    return _latest_state[0].last_active_tile_fraction()


# torch.autograd.Function.apply first scans every argument for functorch wrappers (30-35 us for the ~80 arguments of a
# colour-stage call); no transform is ever active on this path, so the C-level apply is bound directly.  Falls back to the
# public entry when the private attribute is missing or a functorch transform IS active.
try:
    _render_apply = torch._C._FunctionBase.__dict__['apply'].__get__(None, _RenderFn)
except Exception:           # pragma: no cover
    _render_apply = None


# ------------------------------------------------------------------------------------------------
# step plans: the Python-driven call with its host work cached (include/enslam_hip.h, "Step plans")
# ------------------------------------------------------------------------------------------------
# A render call of a loop repeats with the same tensors (the optimiser changes their values in place): everything the host
# derives from them -- which grids convert, where every buffer lies, the parameter pointer tables -- is built once into an
# enslam_step_plan and found again by identity; a call then allocates three blobs and makes ONE library call per direction
# (0.2 ms of Python per direction before).  Taken for plain calls only: sampled rays with gt_depth, whole 16-sample tiles, no
# hipGraph capture of this library in progress (its persistent gradients are _RenderFn's), no VoxelMajorGrid, no given sample
# distances, no per-kernel profiling.  ENSLAM_STEP_PLANS=0 switches it off (same numbers either way).
STEP_PLANS = os.environ.get('ENSLAM_STEP_PLANS', '1') == '1'
_N_PARAMS = 23


class _PlanEntry:
    __slots__ = ('plan', 'layout', 'tensors', 'ptrs', 'rgrad', 'kinds', 'modes', 'dims', 'par_grad', 'need_rays', 'like', 'keep',
                 'n_in', 'flag_spec', 'ntiles')


plan_stats = {'built': 0, 'hits': 0, 'declined': 0}      # (diagnostic counters; tests read them)
# > 0 while graph.GraphedStep runs the eager warm-up iterations of a step it is about to capture: those must leave the caches the
# capture will read (packed decoders of fixed decoders, converted grids) warm, which only _RenderFn's route fills
plans_suspended = [0]
_plan_entries = {}              # (stage, N, n_lin, n_surf, lindisp, loss key, work list, t_lin ptr, t_surf ptr, bound key) -> [entries]


def _plan_build(rplan, N, rays_o, rays_d, grids, params_flat, loss_key):
    lib = L.lib()
    e = _PlanEntry()
    P, kinds = L.StepPlan(), rplan.kinds
    nk = len(kinds)
    P.stage, P.n_rays, P.n_lin, P.n_surf, P.lindisp = L.STAGE[rplan.stage], N, rplan.n_lin, rplan.n_surf, rplan.lindisp
    P.need_rays = int(rays_o.requires_grad or rays_d.requires_grad)
    P.use_work_list = int(rplan.state.use_work_list)
    P.loss_kind, P.use_color, P.w_color = loss_key
    e.modes, e.dims, e.par_grad, like = {}, {}, {}, []
    po = 0
    off = 0
    for i, k in enumerate(kinds):
        g = grids[i]
        _check_grid(g)
        nat = is_native_grid(g)
        e.modes[k] = (2 if nat else 3) if g.requires_grad else 1
        e.dims[k] = tuple(int(x) for x in g.shape[2:])
        P.grid_mode[k] = e.modes[k]
        P.grid_D[k], P.grid_H[k], P.grid_W[k] = e.dims[k]
        ps = params_flat[po:po + _N_PARAMS]
        po += _N_PARAMS
        _check_params(k, ps)
        P.params[k] = _fill_params_struct(k, ps)
        e.par_grad[k] = any(p.requires_grad for p in ps)
        P.par_grad[k] = int(e.par_grad[k])
        if e.par_grad[k]:
            for j, t in enumerate(ps):
                P.pgrad_off[k][j] = off
                off += t.numel()
            like += list(ps)
    P.pgrad_floats = off
    P.act_light = int(not any(e.par_grad.values()))
    P.bound, P.coarse_bound = rplan.bound6, rplan.coarse_bound6
    P.t_lin, P.t_surf = _ptr(rplan.t_lin), _ptr(rplan.t_surf)
    Lay = L.StepLayout()
    rc = lib.enslam_plan_layout(ctypes.byref(P), ctypes.byref(Lay))
    if rc != 0:
        return None
    n_act = _lib_size('enslam_activation_floats', P.stage, N, Lay.n_samples, P.act_light)
    if not (0 < n_act * 4 <= ACT_WORKSPACE_LIMIT_BYTES) or max(d[0] * d[1] * d[2] for d in e.dims.values()) >= (1 << 29):
        return None
    e.plan, e.layout, e.kinds, e.like, e.need_rays = P, Lay, kinds, like, bool(P.need_rays)
    # (grids by weak reference: a cached plan must not keep a replaced 45 MB map alive; the decoders' parameters are small)
    e.tensors = [weakref.ref(g) for g in grids] + list(params_flat)
    e.ptrs = [t.data_ptr() for t in params_flat] + [rplan.t_lin.data_ptr(), rplan.t_surf.data_ptr() if rplan.t_surf is not None else 0]
    e.rgrad = [t.requires_grad for t in [rays_o, rays_d] + list(grids) + list(params_flat)]
    e.keep = (rplan.t_lin, rplan.t_surf)
    e.n_in = 4 + nk + len(params_flat)
    e.ntiles = N * (Lay.n_samples // 16)
    return e


def _plan_lookup(rplan, N, rays_o, rays_d, grids, params_flat, loss_key):
    tl, ts = rplan.t_lin, rplan.t_surf
    key = (rplan.stage, N, rplan.n_lin, rplan.n_surf, rplan.lindisp, loss_key, rplan.state.use_work_list, id(rplan.state),
           tuple(rplan.bound6), tuple(rplan.coarse_bound6))
    lst = _plan_entries.get(key)
    tensors = [rays_o, rays_d] + list(grids) + list(params_flat)
    nk = len(grids)
    if lst is not None:
        for e in lst:
            t0 = e.tensors
            # rays may be new tensors every step (only their gradient flag matters); grids and parameters are found by identity
            if len(t0) + 2 == len(tensors) and all(r() is g for r, g in zip(t0[:nk], grids)) and \
                    all(a is b for a, b in zip(t0[nk:], params_flat)) and \
                    e.rgrad == [t.requires_grad for t in tensors] and \
                    e.ptrs == [t.data_ptr() for t in params_flat] + [tl.data_ptr(), ts.data_ptr() if ts is not None else 0] and \
                    all(tuple(g.shape[2:]) == e.dims[k] and ((e.modes[k] == 3) != is_native_grid(g) or e.modes[k] == 1)
                        for g, k in zip(grids, rplan.kinds)):
                plan_stats['hits'] += 1
                return e
    e = _plan_build(rplan, N, rays_o, rays_d, grids, params_flat, loss_key)
    if e is None:
        plan_stats['declined'] += 1
        return None
    plan_stats['built'] += 1
    if len(_plan_entries) > 64:
        _plan_entries.clear()
    _plan_entries.setdefault(key, []).insert(0, e)
    del _plan_entries[key][4:]
    return e


def _blob_view(blob, off, nbytes, dtype):
    return blob[off:off + nbytes].view(dtype)


class _PlanFn(torch.autograd.Function):
    """_RenderFn for calls served by a step plan: inputs (entry, rplan, rays_o, rays_d, gt_depth, gt_color | None, *grids, *params)."""

    @staticmethod
    def forward(ctx, e, rplan, rays_o, rays_d, gt_depth, gt_color, *tensors):
        lib = L.lib()
        ctx.set_materialize_grads(False)
        P, Lay = e.plan, e.layout
        nk = len(e.kinds)
        dev = rays_o.device
        ro, rd = _f32c(rays_o), _f32c(rays_d)
        gd = _f32c(gt_depth).reshape(-1)
        gc = gt_color                               # (already detached contiguous float32 [N,3] or None: Renderer)
        u8 = torch.uint8
        scratch = torch.empty(Lay.scratch_bytes, dtype=u8, device=dev)
        gradb = torch.empty(Lay.grad_bytes, dtype=u8, device=dev)
        outb = torch.empty(Lay.out_bytes, dtype=u8, device=dev)
        gv = (ctypes.c_void_p * 4)()
        hold = []
        static = [(i, k) for i, k in enumerate(e.kinds) if e.modes[k] == 1 and not is_native_grid(tensors[i])]
        if static:
            for (i, k), vm in zip(static, _grid_cache.get_many([tensors[i] for i, _ in static])):
                gv[k] = vm.data_ptr()
                hold.append(vm)
        for i, k in enumerate(e.kinds):
            if gv[k]:
                continue
            g = tensors[i].detach()
            if e.modes[k] == 3 and not g.is_contiguous():
                g = g.contiguous()
            gv[k] = g.data_ptr()
            hold.append(g)
        st = _stream()
        L.check(lib.enslam_plan_forward(ctypes.byref(P), ctypes.byref(Lay), scratch.data_ptr(), gradb.data_ptr(), outb.data_ptr(),
                                        _ptr(ro), _ptr(rd), _ptr(gd), _ptr(gc), _ptr(rplan.depth_max), gv, st), "enslam_plan_forward")
        N = P.n_rays
        depth = _blob_view(outb, Lay.o_depth, 8 * N, torch.float64)
        var = _blob_view(outb, Lay.o_var, 8 * N, torch.float64)
        rgb = _blob_view(outb, Lay.o_rgb, 12 * N, torch.float32).view(N, 3)
        state = rplan.state
        _latest_state[0] = state
        state.flags = {}
        for i, k in enumerate(e.kinds):
            if e.modes[k] >= 2:
                state.flags[id(tensors[i])] = scratch[Lay.s_flags[k]:Lay.s_flags[k] + (e.dims[k][0] * e.dims[k][1] * e.dims[k][2] + 63) // 64]
        state.work = (_blob_view(gradb, Lay.g_counter, 4, torch.int32), e.ntiles) if P.use_work_list else (None, 0)
        ctx.e, ctx.rplan = e, rplan
        ctx.keep = (ro, rd, gd, gc, scratch, gradb, outb, gv, hold)
        ctx.live_guard = _live_grid_guard(tensors[:len(e.kinds)]) if any(ctx.needs_input_grad) else []
        ctx.calls = 0
        if P.loss_kind == 1:
            loss = _blob_view(outb, Lay.o_loss, 8, torch.float64)
            ctx.mark_non_differentiable(depth, var, rgb)
            return loss[0], depth, var, rgb
        return depth, var, rgb

    @staticmethod
    def backward(ctx, *gouts):
        lib = L.lib()
        e = ctx.e
        P, Lay = e.plan, e.layout
        ro, rd, gd, gc, scratch, gradb, outb, gv, hold = ctx.keep
        _check_live_grids(ctx.live_guard)
        N, dev = P.n_rays, ro.device
        n_in = e.n_in + 2
        if P.loss_kind == 1:
            g_loss, g_depth, g_var, g_rgb = gouts[0], None, None, None
        else:
            g_loss = None
            g_depth, g_var, g_rgb = gouts

        def prep(g, dtype, shape):
            if g is None:
                return None
            g = g.detach()
            if g.dtype is not dtype:
                g = g.to(dtype)
            if tuple(g.shape) != shape:
                g = g.expand(shape)
            return g if g.is_contiguous() else g.contiguous()

        gD, gV, gC = prep(g_depth, torch.float64, (N,)), prep(g_var, torch.float64, (N,)), prep(g_rgb, torch.float32, (N, 3))
        gL = prep(g_loss, torch.float64, (1,))
        if gD is None and gV is None and gC is None and gL is None:
            return (None,) * n_in
        st = _stream()
        if ctx.calls > 0:
            # a repeated backward of this call (retain_graph): the first one's gradient blob backs tensors it returned -- this
            # one adds into a fresh, cleared blob (the work list of a fused-loss forward keeps its counter) and cleared
            # channel-major accumulators
            old = gradb
            gradb = torch.zeros(Lay.grad_bytes, dtype=torch.uint8, device=dev)
            if P.loss_kind == 1 and P.use_work_list:
                gradb[Lay.g_counter:Lay.g_counter + 4].copy_(old[Lay.g_counter:Lay.g_counter + 4])
            m3 = [k for k in e.kinds if e.modes[k] == 3]
            if m3:
                n = len(m3)
                dsts, vs, nd = (ctypes.c_void_p * n)(), (ctypes.c_int64 * n)(), (ctypes.c_void_p * n)()
                for j, k in enumerate(m3):
                    dsts[j] = scratch.data_ptr() + Lay.s_gacc[k]
                    vs[j] = e.dims[k][0] * e.dims[k][1] * e.dims[k][2]
                    nd[j] = scratch.data_ptr() + Lay.s_flags[k]
                L.check(lib.enslam_zero_blocks(n, dsts, vs, nd, None, 0, st), "enslam_zero_blocks")
        ctx.calls += 1
        L.check(lib.enslam_plan_backward(ctypes.byref(P), ctypes.byref(Lay), scratch.data_ptr(), gradb.data_ptr(), outb.data_ptr(),
                                         _ptr(ro), _ptr(rd), _ptr(gd), _ptr(gc), gv, _ptr(gD), _ptr(gV), _ptr(gC), _ptr(gL), st),
                "enslam_plan_backward")
        needs = ctx.needs_input_grad
        out = [None, None, None, None, None, None]      # (entry, rplan, rays_o, rays_d, gt_depth, gt_color)
        if e.need_rays:
            if needs[2]:
                out[2] = _blob_view(gradb, Lay.g_ro, 12 * N, torch.float32).view(N, 3)
            if needs[3]:
                out[3] = _blob_view(gradb, Lay.g_rd, 12 * N, torch.float32).view(N, 3)
        for k in e.kinds:
            D, H, W = e.dims[k]
            V = D * H * W
            if e.modes[k] == 2:
                out.append(_native_grad_view(_blob_view(gradb, Lay.g_nat[k], 128 * V, torch.float32), e.dims[k]))
            elif e.modes[k] == 3:
                out.append(_blob_view(gradb, Lay.g_dense[k], 128 * V, torch.float32).view(1, 32, D, H, W))
            else:
                out.append(None)
        if e.like:
            views = torch._C._nn.unflatten_dense_tensors(_blob_view(gradb, Lay.g_params, 4 * P.pgrad_floats, torch.float32), e.like)
            vo = 0
            for k in e.kinds:
                if e.par_grad[k]:
                    out += list(views[vo:vo + _N_PARAMS])
                    vo += _N_PARAMS
                else:
                    out += [None] * _N_PARAMS
        else:
            out += [None] * (_N_PARAMS * len(e.kinds))
        return tuple(out)


try:
    _plan_apply = torch._C._FunctionBase.__dict__['apply'].__get__(None, _PlanFn)
except Exception:           # pragma: no cover
    _plan_apply = None


def _plan_render(plan, rays_o, rays_d, gt_depth, t_rand, grids, params_flat):
    """-> outputs of _PlanFn, or None when the call is not one a step plan serves."""
    if (not STEP_PLANS or _capture['active'] or plans_suspended[0] or plan.z_given is not None or t_rand is not None or gt_depth is None or plan.vm
            or plan.stage == 'coarse' or plan.state.profile or not rays_o.is_cuda or not torch.is_grad_enabled()):
        return None
    N = rays_o.shape[0]
    S = plan.n_lin + plan.n_surf
    if N <= 0 or S % 16 != 0 or S > 64 or len(params_flat) != _N_PARAMS * len(plan.kinds):
        return None
    loss_key, gc = (0, 0, 0.0), None
    if plan.loss is not None:
        if len(plan.loss) != 3:
            return None
        lgd, gc, lw = plan.loss
        if lgd.shape[0] != N:
            return None
        loss_key = (1, int(gc is not None), float(lw))
    if not any(t.requires_grad for t in grids) and not any(t.requires_grad for t in params_flat) and \
            not (rays_o.requires_grad or rays_d.requires_grad):
        return None                                 # (forward-only calls: nothing to save; _RenderFn's route is as cheap)
    e = _plan_lookup(plan, N, rays_o, rays_d, grids, params_flat, loss_key)
    if e is None:
        return None
    if _plan_apply is not None and not torch._C._are_functorch_transforms_active():
        return _plan_apply(e, plan, rays_o, rays_d, gt_depth, gc, *grids, *params_flat)
    return _PlanFn.apply(e, plan, rays_o, rays_d, gt_depth, gc, *grids, *params_flat)


def render(plan, rays_o, rays_d, gt_depth, t_rand, grids, params_flat):
    out = _plan_render(plan, rays_o, rays_d, gt_depth, t_rand, grids, params_flat)
    if out is not None:
        return out
    if _render_apply is not None and not torch._C._are_functorch_transforms_active():
        return _render_apply(plan, rays_o, rays_d, gt_depth, t_rand, *grids, *params_flat)
    return _RenderFn.apply(plan, rays_o, rays_d, gt_depth, t_rand, *grids, *params_flat)


# ------------------------------------------------------------------------------------------------
# forward-only helpers
# ------------------------------------------------------------------------------------------------
def eval_points(p, decoders, c, stage, bound, apply_mask=True, coarse_bound=None):
    """raw [P,4] float32 for points p [P,3] (any float dtype; evaluated as float64 like the reference)."""
    lib = L.lib()
    _require_hip(p, "points")
    if torch.is_grad_enabled() and (p.requires_grad or any(
            c[L.GRID_NAMES[k]].requires_grad for k in stage_kinds(stage))):
        raise NotImplementedError("eval_points is forward-only on the HIP path (its differentiable use, "
                                  "Renderer.regulation, belongs to the iMAP mode); wrap the call in torch.no_grad()")
    pts = p.detach().to(torch.float64).contiguous()
    P = pts.shape[0]
    kinds = stage_kinds(stage)
    grids_vm, dims, packed = {}, {}, {}
    for k in kinds:
        g = c[L.GRID_NAMES[k]]
        grids_vm[k] = g.vm if isinstance(g, VoxelMajorGrid) else _grid_cache.get(g)
        dims[k] = tuple(g.shape[2:])
        packed[k] = packed_decoder(getattr(decoders, L.MLP_NAMES[k]), k)
    if coarse_bound is None:
        coarse_bound = decoders.coarse_decoder.bound if 0 in kinds else bound
    sc = _scene_struct(stage, bound6(bound), bound6(coarse_bound), grids_vm, dims, packed)
    raw = torch.empty((P, 4), dtype=torch.float32, device=p.device)
    L.check(lib.enslam_eval_points(L.STAGE[stage], P, _ptr(pts), ctypes.byref(sc), int(apply_mask), _ptr(raw),
                                   _stream()), "enslam_eval_points")
    return raw


def voxel_index(points, bound, shape):
    """Parity helper: (ix,iy,iz int32, fx,fy,fz float32) the gather uses for float64 points [P,3]."""
    lib = L.lib()
    pts = points.detach().to(torch.float64).contiguous()
    P, dev = pts.shape[0], pts.device
    outs = [torch.empty(P, dtype=torch.int32, device=dev) for _ in range(3)] + \
           [torch.empty(P, dtype=torch.float32, device=dev) for _ in range(3)]
    D, H, W = shape
    L.check(lib.enslam_voxel_index(P, _ptr(pts), bound6(bound), D, H, W, *[_ptr(t) for t in outs], _stream()),
            "enslam_voxel_index")
    return outs


def gather_pixels(idx, H0, W0, ww, depth, color):
    """(pix_i, pix_j, depth samples, colour samples) of the window pixels `idx` (int64 [n], row-major inside the window that
    starts at (H0, W0) and is ww wide): what common.get_sample_uv computes with 2 linspace + 2 index-arithmetic + 4 indexing
    launches, in one (enslam_gather_pixels).  depth float32 [H, W], color float32 / float64 [H, W, 3], all on the GPU."""
    n = int(idx.shape[0])
    dev = idx.device
    depth, color, idx = depth.contiguous(), color.contiguous(), idx.contiguous()
    oi = torch.empty(n, dtype=torch.float32, device=dev)
    oj = torch.empty(n, dtype=torch.float32, device=dev)
    od = torch.empty(n, dtype=torch.float32, device=dev)
    oc = torch.empty((n, 3), dtype=color.dtype, device=dev)
    L.check(L.lib().enslam_gather_pixels(n, _ptr(idx), int(H0), int(W0), int(ww), int(depth.shape[1]), int(depth.shape[0]), _ptr(depth),
                                         _ptr(color), int(color.dtype == torch.float64), _ptr(oi), _ptr(oj), _ptr(od), _ptr(oc),
                                         _stream()), "enslam_gather_pixels")
    return oi, oj, od, oc


def gather_pixels_ok(idx, depth, color):
    return (idx.is_cuda and depth.is_cuda and color.is_cuda and idx.dtype == torch.int64 and depth.dtype == torch.float32
            and depth.dim() == 2 and color.dim() == 3 and color.shape[2] == 3 and tuple(color.shape[:2]) == tuple(depth.shape)
            and color.dtype in (torch.float32, torch.float64) and not depth.requires_grad and not color.requires_grad)


def fourier_sincos(x):
    """Parity helper: (sin, cos) float32 of float32 arguments as the embedding kernels evaluate them."""
    _require_hip(x, "x")
    xx = x.detach().contiguous().float().reshape(-1)
    s, c = torch.empty_like(xx), torch.empty_like(xx)
    L.check(L.lib().enslam_fourier_sincos(xx.numel(), _ptr(xx), _ptr(s), _ptr(c), _stream()), "enslam_fourier_sincos")
    return s.reshape(x.shape), c.reshape(x.shape)


def ray_points(rays_o, rays_d, z_vals, bound):
    """Parity helper: float64 sample points [N*S,3] and the strict in-bound mask."""
    lib = L.lib()
    N, S = z_vals.shape
    pts = torch.empty((N * S, 3), dtype=torch.float64, device=z_vals.device)
    mask = torch.empty(N * S, dtype=torch.uint8, device=z_vals.device)
    L.check(lib.enslam_ray_points(N, S, _ptr(rays_o.contiguous().float()), _ptr(rays_d.contiguous().float()),
                                  _ptr(z_vals.contiguous()), bound6(bound), _ptr(pts), _ptr(mask), _stream()),
            "enslam_ray_points")
    return pts, mask.bool()


def sample_rays(rays_o, rays_d, gt_depth, bound, n_lin, n_surf, lindisp=False, t_rand=None, depth_max=None):
    """z_vals float64 [N,S] (Renderer.py:83-171)."""
    lib = L.lib()
    _require_hip(rays_o, "rays")
    N, dev = rays_o.shape[0], rays_o.device
    S = n_lin + (n_surf if gt_depth is not None else 0)
    t_lin = torch.linspace(0., 1., steps=n_lin, device=dev)
    t_surf = torch.linspace(0., 1., steps=max(n_surf, 1), device=dev).double() if n_surf > 0 else None
    z = torch.empty((N, S), dtype=torch.float64, device=dev)
    scratch = torch.empty(2, dtype=torch.float32, device=dev)
    gd = gt_depth.contiguous().float().reshape(-1) if gt_depth is not None else None
    if depth_max is not None:
        scratch = depth_max
    L.check(lib.enslam_sample_rays(N, n_lin, n_surf, _ptr(rays_o.contiguous().float()),
                                   _ptr(rays_d.contiguous().float()), _ptr(gd), bound6(bound), _ptr(t_lin),
                                   _ptr(t_surf), int(bool(lindisp)), _ptr(t_rand), _ptr(scratch),
                                   int(depth_max is not None), _ptr(z), 0, None, None, _stream()), "enslam_sample_rays")
    return z


def batch_depth_max(gt_depth):
    """{max(gt_depth), fl32(max*1.2)} float32 [2]: what a ray-sharded caller passes to every shard
    (Renderer.py:110,145 take these maxima over the whole batch)."""
    m = gt_depth.detach().float().max().reshape(1)
    return torch.cat([m, m * 1.2]).contiguous()


class _CompositeFn(torch.autograd.Function):
    """raw2outputs_nerf_color with occupancy=True as one HIP kernel each way; gradient to `raw` only."""

    @staticmethod
    def forward(ctx, raw, z_vals):
        lib = L.lib()
        _require_hip(raw, "raw")
        N, S = z_vals.shape
        if S > 64:
            raise L.EnslamError("composite kernels handle at most 64 samples per ray")
        r = raw.detach().contiguous().float()
        z = z_vals.detach().contiguous().double()
        dev = raw.device
        depth = torch.empty(N, dtype=torch.float64, device=dev)
        var = torch.empty(N, dtype=torch.float64, device=dev)
        rgb = torch.empty((N, 3), dtype=torch.float32, device=dev)
        w = torch.empty((N, S), dtype=torch.float32, device=dev)
        L.check(lib.enslam_composite_fwd(N, S, _ptr(r), _ptr(z), _ptr(depth), _ptr(var), _ptr(rgb), _ptr(w), _stream()),
                "enslam_composite_fwd")
        ctx.keep = (r, z, depth)
        ctx.mark_non_differentiable(w)
        return depth, var, rgb, w

    @staticmethod
    def backward(ctx, g_depth, g_var, g_rgb, _gw):
        lib = L.lib()
        r, z, depth = ctx.keep
        N, S = z.shape
        gD = g_depth.detach().double().contiguous() if g_depth is not None else None
        gV = g_var.detach().double().contiguous() if g_var is not None else None
        gC = g_rgb.detach().float().contiguous() if g_rgb is not None else None
        d_raw = torch.empty((N, S, 4), dtype=torch.float32, device=r.device)
        L.check(lib.enslam_composite_bwd(N, S, _ptr(r), _ptr(z), _ptr(depth), _ptr(gD), _ptr(gV), _ptr(gC),
                                         _ptr(d_raw), _stream()), "enslam_composite_bwd")
        return d_raw, None


def composite(raw, z_vals):
    """(depth f64 [N], var f64 [N], rgb f32 [N,3], weights f32 [N,S]) from raw [N,S,4], z_vals [N,S]."""
    return _CompositeFn.apply(raw, z_vals)


def marching_cubes(volume, level, origin, spacing):
    """(verts float64 [V,3], faces int32 [F,3]) of the level set `value = level` of a lattice volume [nx, ny, nz] (z fastest,
    evaluated as float32) whose point [ix, iy, iz] sits at origin + index * spacing: skimage.measure.marching_cubes as
    Mesher.py:495-520 calls it, plus its `verts + origin`.  Conventions (vertex order, winding, case table): enslam_hip.h.
    One host synchronisation: the counts, so the outputs are allocated exactly."""
    lib = L.lib()
    _require_hip(volume, "volume")
    if volume.dim() != 3:
        raise L.EnslamError(f"marching_cubes wants a [nx, ny, nz] volume (got shape {tuple(volume.shape)})")
    vol = _f32c(volume)
    nx, ny, nz = (int(n) for n in vol.shape)
    dev = vol.device
    nbytes = ctypes.c_int64()
    L.check(lib.enslam_marching_cubes_workspace(nx, ny, nz, ctypes.byref(nbytes)), "enslam_marching_cubes_workspace")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    L.check(lib.enslam_marching_cubes_count(_ptr(vol), nx, ny, nz, float(level), _ptr(ws), _ptr(counts), _stream()),
            "enslam_marching_cubes_count")
    n_verts, n_faces = counts.tolist()
    verts = torch.empty((n_verts, 3), dtype=torch.float64, device=dev)
    faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
    org = (ctypes.c_double * 3)(*[float(x) for x in origin])
    spc = (ctypes.c_double * 3)(*[float(x) for x in spacing])
    L.check(lib.enslam_marching_cubes_emit(_ptr(vol), nx, ny, nz, float(level), org, spc, _ptr(ws), n_verts, n_faces,
                                           _ptr(verts), _ptr(faces), _stream()), "enslam_marching_cubes_emit")
    return verts, faces


def world_to_camera(c2w_list):
    """float64 numpy [K,3,4]: the upper rows of the inverses of the camera-to-world matrices, inverted on the host in float64 as
    the reference does (np.linalg.inv of the pose's numpy form)."""
    import numpy as np
    out = np.zeros((len(c2w_list), 3, 4), np.float64)
    for k, c2w in enumerate(c2w_list):
        m = c2w.detach().cpu().numpy() if torch.is_tensor(c2w) else np.asarray(c2w)
        out[k] = np.linalg.inv(m.astype(np.float64))[:3]
    return out


def visibility(points, w2c, cam, edge_seen=0, edge_forecast=-1000, z_eps=1e-8, limit=None, depth=None, lattice=None,
               first=0, count=None, want_classes=True, want_counts=False, dtype=torch.float32):
    """Classes and per-camera counts of points against K cameras (enslam_visibility, enslam_hip.h; Mesher.py:88-190 and
    Mapper.py:218-241).
      points    float32 [P,3] on a HIP device, or None with lattice=(ax, ay, az) float32 device axes: the `count` points from
                linear index `first` of the lattice in Mesher.lattice_volume's order
      w2c       world-to-camera matrices [K,3,4] or [K,4,4] (numpy or tensor, see world_to_camera); they are rounded to `dtype`
      cam       dict with H, W, fx, fy, cx, cy
      limit     float32 [K] per-camera bound on the projected depth, or None
      depth     float32 [K,H,W] depth images for the depth test, or None
      dtype     torch.float32 (the Mesher's arithmetic) or torch.float64 (the overlap selection's)
    Returns (classes uint8 [P] or None, counts int32 [K] or None); classes: 0 unseen, 1 seen, 2 forecast.  The largest depth
    sample the forecast test uses is taken over the points of THIS call, so chunk as the reference chunks."""
    lib = L.lib()
    if dtype not in (torch.float32, torch.float64):
        raise L.EnslamError(f"visibility computes in float32 or float64 (got {dtype})")
    if (points is None) == (lattice is None):
        raise L.EnslamError("visibility wants either explicit points or a lattice")
    if points is not None:
        _require_hip(points, "points")
        if points.dim() != 2 or points.shape[1] != 3:
            raise L.EnslamError(f"points must be [P,3] (got shape {tuple(points.shape)})")
        pts, axes, dims, first = _f32c(points), (None, None, None), (0, 0, 0), 0
        P, dev = int(pts.shape[0]), pts.device
    else:
        for a in lattice:
            _require_hip(a, "lattice axes")
            if a.dim() != 1 or a.shape[0] < 1:
                raise L.EnslamError("lattice axes must be non-empty 1-D tensors")
        pts, axes = None, tuple(_f32c(a) for a in lattice)
        dims = tuple(int(a.shape[0]) for a in axes)
        total = dims[0] * dims[1] * dims[2]
        P, dev = (total - int(first)) if count is None else int(count), axes[0].device
        if first < 0 or P < 0 or first + P > total:
            raise L.EnslamError(f"lattice range [{first}, {first + P}) leaves the {total} lattice points")
    w = torch.as_tensor(w2c)
    if w.dim() != 3 or tuple(w.shape[1:]) not in ((3, 4), (4, 4)):
        raise L.EnslamError(f"w2c must be [K,3,4] or [K,4,4] (got shape {tuple(w.shape)})")
    K = int(w.shape[0])
    w = w[:, :3].to(dtype).contiguous().to(dev)
    H, W = int(cam['H']), int(cam['W'])
    lim = dep = ws = None
    if limit is not None:
        _require_hip(limit, "limit")
        lim = _f32c(limit).reshape(-1)
        if lim.shape[0] != K:
            raise L.EnslamError(f"limit has {lim.shape[0]} entries for {K} cameras")
    if depth is not None:
        _require_hip(depth, "depth")
        dep = _f32c(depth)
        if tuple(dep.shape) != (K, H, W):
            raise L.EnslamError(f"depth must be [{K},{H},{W}] (got shape {tuple(dep.shape)})")
        nbytes = ctypes.c_int64()
        L.check(lib.enslam_visibility_workspace(K, ctypes.byref(nbytes)), "enslam_visibility_workspace")
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    classes = torch.empty(P, dtype=torch.uint8, device=dev) if want_classes else None
    counts = torch.empty(K, dtype=torch.int32, device=dev) if want_counts else None
    with torch.cuda.device(dev):
        L.check(lib.enslam_visibility(1 if dtype is torch.float64 else 0, P, _ptr(pts), _ptr(axes[0]), _ptr(axes[1]), _ptr(axes[2]),
                                      dims[0], dims[1], dims[2], int(first), K, _ptr(w) if K else None, float(cam['fx']),
                                      float(cam['fy']), float(cam['cx']), float(cam['cy']), H, W, int(edge_seen),
                                      int(edge_forecast), float(z_eps), _ptr(lim), _ptr(dep), _ptr(ws), _ptr(classes),
                                      _ptr(counts), _stream()), "enslam_visibility")
    return classes, counts


def _mesh_faces(faces, n_verts):
    _require_hip(faces, "faces")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype is not torch.int32:
        raise L.EnslamError(f"faces must be int32 [F,3] (got {faces.dtype} {tuple(faces.shape)})")
    if int(n_verts) < 0:
        raise L.EnslamError(f"n_verts must not be negative (got {n_verts})")
    return faces.detach().contiguous()


def _mesh_workspace(lib, n_verts, n_faces, dev):
    nbytes = ctypes.c_int64()
    L.check(lib.enslam_mesh_clean_workspace(n_verts, n_faces, ctypes.byref(nbytes)), "enslam_mesh_clean_workspace")
    return torch.empty(nbytes.value, dtype=torch.uint8, device=dev)


def mesh_components(faces, n_verts):
    """int32 [F] labels of the edge-connected components of a triangle mesh (faces int32 [F,3] on a HIP device, indices in
    [0, n_verts)): the label of a face is the smallest face index of its component; faces sharing an edge (the same unordered
    vertex pair) are connected, faces sharing only a vertex are not (enslam_hip.h; mesher.face_components is the host form)."""
    lib = L.lib()
    f = _mesh_faces(faces, n_verts)
    F, dev = int(f.shape[0]), f.device
    labels = torch.empty(F, dtype=torch.int32, device=dev)
    if F == 0:
        return labels
    with torch.cuda.device(dev):
        ws = _mesh_workspace(lib, int(n_verts), F, dev)
        L.check(lib.enslam_mesh_components(_ptr(f), F, int(n_verts), _ptr(ws), _ptr(labels), _stream()), "enslam_mesh_components")
    return labels


def mesh_clean(vertices, faces, vertex_keep=None, min_area=0.0, largest_only=False, stats=None):
    """(vertices float64 [V',3], faces int32 [F',3], vertex_index int32 [V']) of a triangle mesh (vertices float64 [V,3], faces
    int32 [F,3], HIP device) after the cleaning of Mesher.get_mesh: faces none of whose vertices is kept by vertex_keep (bool /
    uint8 [V], None: keep all) go, then every edge-connected component whose area is not above min_area (or, with largest_only,
    every component but the largest), then the vertices no face uses.  Faces and vertices keep their order; vertex_index is the
    original index of each kept vertex.  Bit-equal to mesher.drop_unreferenced(v, mesher.filter_components(v, f_masked, ...))
    unless a component's area is within rounding of the threshold (enslam_hip.h).  One host synchronisation: the counts.
    `stats`, a dict, receives the number of components after the mask drop."""
    lib = L.lib()
    _require_hip(vertices, "vertices")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype is not torch.float64:
        raise L.EnslamError(f"vertices must be float64 [V,3] (got {vertices.dtype} {tuple(vertices.shape)})")
    v = vertices.detach().contiguous()
    V, dev = int(v.shape[0]), v.device
    f = _mesh_faces(faces, V)
    F = int(f.shape[0])
    keep = None
    if vertex_keep is not None:
        _require_hip(vertex_keep, "vertex_keep")
        if vertex_keep.dtype not in (torch.bool, torch.uint8) or tuple(vertex_keep.shape) != (V,):
            raise L.EnslamError(f"vertex_keep must be bool or uint8 [{V}] (got {vertex_keep.dtype} {tuple(vertex_keep.shape)})")
        keep = vertex_keep.detach().contiguous()
        keep = keep.view(torch.uint8) if keep.dtype is torch.bool else keep
    if f.device != dev or (keep is not None and keep.device != dev):
        raise L.EnslamError("vertices, faces and vertex_keep must live on one device")
    if F == 0:
        if stats is not None:
            stats['components'] = 0
        return v.new_empty((0, 3)), f.new_empty((0, 3)), torch.empty(0, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws = _mesh_workspace(lib, V, F, dev)
        counts = torch.empty(3, dtype=torch.int32, device=dev)
        L.check(lib.enslam_mesh_clean_count(_ptr(v), V, _ptr(f), F, _ptr(keep), float(min_area), 1 if largest_only else 0,
                                            _ptr(ws), _ptr(counts), _stream()), "enslam_mesh_clean_count")
        n_v, n_f, n_comp = counts.tolist()
        v_out = torch.empty((n_v, 3), dtype=torch.float64, device=dev)
        f_out = torch.empty((n_f, 3), dtype=torch.int32, device=dev)
        index = torch.empty(n_v, dtype=torch.int32, device=dev)
        L.check(lib.enslam_mesh_clean_emit(_ptr(v), V, _ptr(f), F, _ptr(ws), n_v, n_f, _ptr(v_out), _ptr(f_out), _ptr(index),
                                           _stream()), "enslam_mesh_clean_emit")
    if stats is not None:
        stats['components'] = n_comp
    return v_out, f_out, index


NN_DEFAULT_MAX_RINGS = 4     # Chebyshev shells a query walks before the brute-force kernel takes it over


def _points64(t, what):
    _require_hip(t, what)
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype is not torch.float64:
        raise L.EnslamError(f"{what} must be float64 [N,3] (got {t.dtype} {tuple(t.shape)})")
    t = t.detach().contiguous()
    if not bool(torch.isfinite(t).all()):
        raise L.EnslamError(f"{what} holds non-finite coordinates")
    return t


class NearestIndex:
    """The cell grid of enslam_nn_build over a reference point set (float64 [N,3], HIP device), for any number of queries --
    the ICP of eval_recon.align_icp builds it once for its 30 iterations."""

    def __init__(self, ref):
        self.lib = L.lib()
        self.ref = _points64(ref, "ref")
        self.N, self.device = int(self.ref.shape[0]), self.ref.device
        if self.N == 0:
            raise L.EnslamError("nearest needs at least one reference point")
        self.ws = None

    def _grid(self):
        if self.ws is None:
            nbytes = ctypes.c_int64()
            L.check(self.lib.enslam_nn_workspace(self.N, 0, ctypes.byref(nbytes), None), "enslam_nn_workspace")
            self.ws = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
            L.check(self.lib.enslam_nn_build(_ptr(self.ref), self.N, _ptr(self.ws), _stream()), "enslam_nn_build")
        return self.ws

    def query(self, query, max_dist=None, max_rings=None, stats=None):
        """(dist float64 [M], idx int32 [M]); `stats`, a dict, receives 'tail': the number of queries the brute-force kernel
        finished (one host synchronisation, only when asked for)."""
        q = _points64(query, "query")
        if q.device != self.device:
            raise L.EnslamError("query and ref must live on one device")
        rings = NN_DEFAULT_MAX_RINGS if max_rings is None else int(max_rings)
        md = float('inf') if max_dist is None else float(max_dist)
        if rings < 0 or md != md:
            raise L.EnslamError(f"nearest: max_rings must not be negative and max_dist not NaN (got {max_rings}, {max_dist})")
        M = int(q.shape[0])
        dist = torch.empty(M, dtype=torch.float64, device=self.device)
        idx = torch.empty(M, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            grid = qws = None
            if rings > 0 and M > 0:
                grid = self._grid()
                nbytes = ctypes.c_int64()
                L.check(self.lib.enslam_nn_workspace(self.N, M, None, ctypes.byref(nbytes)), "enslam_nn_workspace")
                qws = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
            tail = torch.zeros(1, dtype=torch.int32, device=self.device) if stats is not None else None
            L.check(self.lib.enslam_nn_query(_ptr(self.ref), self.N, _ptr(q), M, md, rings, _ptr(grid), _ptr(qws), _ptr(dist),
                                             _ptr(idx), _ptr(tail), _stream()), "enslam_nn_query")
        if stats is not None:
            stats['tail'] = int(tail.item())
        return dist, idx


def nearest(query, ref, max_dist=None, max_rings=None, stats=None):
    """(dist float64 [M], idx int32 [M]): for every query point (float64 [M,3]) the nearest of the reference points (float64
    [N,3], both on one HIP device), exactly: dist is sqrt((dx*dx + dy*dy) + dz*dz) in float64 in this order -- the bits of
    numpy's np.sqrt(((q - r) ** 2).sum(-1)) -- and among reference points at the same distance the smallest index wins
    (enslam_nn_query, enslam_hip.h).  max_dist: a query with no reference point closer than max_dist gets idx -1 and dist inf.
    max_rings: shells of the cell grid a query walks before the brute-force kernel finishes it (default 4; 0: brute force
    alone); the result does not depend on it.  Non-finite coordinates raise."""
    return NearestIndex(ref).query(query, max_dist=max_dist, max_rings=max_rings, stats=stats)


def _mesh_args(what, vertices, faces):
    """(lib, vertices, V, faces, F, device) of the mesh of `what`: float64 [V,3] and int32 [F,3], contiguous, on one HIP device"""
    if not vertices.is_cuda:
        raise NotImplementedError(f"{what} needs a HIP device")
    lib = L.lib()
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype is not torch.float64:
        raise L.EnslamError(f"vertices must be float64 [V,3] (got {vertices.dtype} {tuple(vertices.shape)})")
    v = vertices.detach().contiguous()
    f = _mesh_faces(faces, v.shape[0])
    if f.device != v.device:
        raise L.EnslamError("vertices and faces must live on one device")
    return lib, v, int(v.shape[0]), f, int(f.shape[0]), v.device


def _views(w2c, cam, dev):
    """(w2c float64 [K,3,4] on dev, K, H, W, (fx, fy, cx, cy)) of K cameras ([K,3,4] or [K,4,4], numpy or tensor) and a cam dict"""
    w = torch.as_tensor(w2c)
    if w.dim() != 3 or tuple(w.shape[1:]) not in ((3, 4), (4, 4)):
        raise L.EnslamError(f"w2c must be [K,3,4] or [K,4,4] (got shape {tuple(w.shape)})")
    w = w[:, :3].to(torch.float64).contiguous().to(dev)
    return w, int(w.shape[0]), int(cam['H']), int(cam['W']), tuple(float(cam[k]) for k in ('fx', 'fy', 'cx', 'cy'))


def mesh_depth(vertices, faces, w2c, cam, z_near=0.0, z_far=20.0):
    """float32 [K,H,W] depth images of a triangle mesh (vertices float64 [V,3], faces int32 [F,3], HIP device) from the K
    cameras w2c ([K,3,4] or [K,4,4], numpy or tensor, the convention of `visibility` / `world_to_camera`: the camera looks
    down -z); cam is a dict with H, W, fx, fy, cx, cy.  Pixel (row j, column i) holds the smallest depth t, z_near < t <=
    z_far, at which the ray through ((i - cx) / fx, -(j - cy) / fy, -1) -- the rays of get_rays and BoxRoom.render -- meets a
    triangle, 0.0 where none does (enslam_mesh_depth, enslam_hip.h): both sides count, edges are inclusive, float64 up to the
    rounding of t.  z_far = 20 is the reference's far plane; z_near = 0 is a difference: the reference's renderer derives
    its near plane from the scene's bounding box."""
    lib, v, V, f, F, dev = _mesh_args("mesh_depth", vertices, faces)
    w, K, H, W, pinhole = _views(w2c, cam, dev)
    depth = torch.empty((K, H, W), dtype=torch.float32, device=dev)
    if K == 0:
        return depth
    with torch.cuda.device(dev):
        nbytes = ctypes.c_int64()
        L.check(lib.enslam_mesh_depth_workspace(F, K, ctypes.byref(nbytes)), "enslam_mesh_depth_workspace")
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        L.check(lib.enslam_mesh_depth(_ptr(v) if V else None, V, _ptr(f) if F else None, F, _ptr(w), K, H, W, *pinhole,
                                      float(z_near), float(z_far), _ptr(ws), _ptr(depth), _stream()), "enslam_mesh_depth")
    return depth


# ------------------------------------------------------------------------------------------------
# Scene rasteriser (csrc/scene_raster.hip): the colour renderer of the headless visualiser (viz.py)
# ------------------------------------------------------------------------------------------------
def vertex_normals(vertices, faces):
    """float64 [V,3]: Open3D's compute_vertex_normals of a mesh on a HIP device (vertices float64 [V,3], faces int32 [F,3]):
    per vertex the unnormalised face normals (b - a) x (c - a) of its incident faces, summed in ascending face order by one
    thread (enslam_scene_normals: the same bits in every run), then normalised; a vertex no face uses, or whose sum is zero,
    gets zero.  A face with an index outside [0, V) is dropped.  The vertex -> face incidence is built here with torch sorts."""
    lib, v, V, f, F, dev = _mesh_args("vertex_normals", vertices, faces)
    out = torch.empty((V, 3), dtype=torch.float64, device=dev)
    if V == 0:
        return out
    with torch.cuda.device(dev):
        ok = ((f >= 0) & (f < V)).all(dim=1)
        vert = f[ok].reshape(-1).to(torch.int64)
        face = torch.arange(F, dtype=torch.int64, device=dev)[ok].repeat_interleave(3)
        order = torch.argsort(vert * max(F, 1) + face)                      # by vertex, then by face: ties are the same face
        inc = face[order].to(torch.int32).contiguous()
        off = torch.zeros(V + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(torch.bincount(vert, minlength=V), 0)
        n_inc = int(inc.shape[0])
        L.check(lib.enslam_scene_normals(_ptr(v), V, _ptr(f) if F else None, F, _ptr(off), _ptr(inc) if n_inc else None, n_inc,
                                         _ptr(out), _stream()), "enslam_scene_normals")
    return out


def scene_raster(vertices, faces, w2c, cam, colors=None, normals=None, points=None, point_colors=None, point_size=4, cull=1,
                 z_near=0.0, z_far=1000.0, ambient=0.35, background=(255, 255, 255), want_depth=False, want_id=False,
                 workspace_bytes=None):
    """uint8 [K,H,W,3] colour images of a triangle mesh (vertices float64 [V,3], faces int32 [F,3]; colors uint8 [V,3] or None:
    0.7 grey; normals float64 [V,3] or None: the face normal) and a point set (points float64 [P,3] with point_colors uint8
    [P,3], or None) on a HIP device, from the K cameras w2c of `mesh_depth`; cam is a dict with H, W, fx, fy, cx, cy
    (enslam_scene_raster, enslam_hip.h).  Per pixel the nearest primitive with z_near < depth <= z_far shows, a face before
    a point at the same float32 depth and the smaller index among equals.  cull: 0 both sides, 1 triangles whose stored
    normal points away from the eye (what the reference's viewer shows), 2 the others.  A point is a point_size x point_size
    square of its colour; a face pixel is its interpolated vertex colour times ambient + (1 - ambient) |n^ . d^|; nothing
    gives `background`.  With want_depth / want_id the result is the tuple (rgb, depth float32 [K,H,W] or None, id int32
    [K,H,W] or None): depth 0 and id -1 where empty, id -2 - p for point p.  workspace_bytes: the size of the scratch
    allocation (default: enslam_scene_raster_workspace); a smaller one shortens the list of large triangles and changes
    nothing in the images."""
    lib, v, V, f, F, dev = _mesh_args("scene_raster", vertices, faces)

    def per(t, n, dtype, what):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (n, 3) or t.dtype is not dtype or t.device != dev:
            raise L.EnslamError(f"{what} must be {dtype} [{n},3] on {dev}")
        return t.detach().contiguous()

    col, nrm = per(colors, V, torch.uint8, "colors"), per(normals, V, torch.float64, "normals")
    P = 0 if points is None else int(points.shape[0])
    pts, pcol = per(points, P, torch.float64, "points"), per(point_colors, P, torch.uint8, "point_colors")
    if (pts is None) != (pcol is None):
        raise L.EnslamError("points and point_colors come together")
    w, K, H, W, pinhole = _views(w2c, cam, dev)
    bg = [int(c) for c in background]
    if len(bg) != 3 or min(bg) < 0 or max(bg) > 255:
        raise L.EnslamError(f"background must be three levels in 0..255 (got {background})")
    rgb = torch.empty((K, H, W, 3), dtype=torch.uint8, device=dev)
    depth = torch.empty((K, H, W), dtype=torch.float32, device=dev) if want_depth else None
    ids = torch.empty((K, H, W), dtype=torch.int32, device=dev) if want_id else None
    with torch.cuda.device(dev):
        nbytes = ctypes.c_int64()
        L.check(lib.enslam_scene_raster_workspace(F, K, H, W, ctypes.byref(nbytes)), "enslam_scene_raster_workspace")
        nbytes = nbytes.value if workspace_bytes is None else int(workspace_bytes)
        ws = torch.empty(max(nbytes, 0), dtype=torch.uint8, device=dev)
        L.check(lib.enslam_scene_raster(_ptr(v) if V else None, V, _ptr(f) if F else None, F, _ptr(col), _ptr(nrm),
                                        _ptr(pts) if P else None, P, _ptr(pcol) if P else None, int(point_size), _ptr(w), K, H, W,
                                        *pinhole, float(z_near), float(z_far), int(cull), float(ambient),
                                        bg[0] | bg[1] << 8 | bg[2] << 16, 7,
                                        _ptr(ws) if nbytes > 0 else None, nbytes, _ptr(rgb), _ptr(depth), _ptr(ids), _stream()),
                "enslam_scene_raster")
    return (rgb, depth, ids) if (want_depth or want_id) else rgb


# ------------------------------------------------------------------------------------------------
# Block-sparse TSDF volume (csrc/tsdf.hip): the raw calls; tsdf.TSDFVolume holds the arrays and allocates
# ------------------------------------------------------------------------------------------------
def _i32x3(v):
    return (ctypes.c_int32 * 3)(*[int(x) for x in v])


def _pose12(m):
    """host float64 [12]: the upper three rows of a [3|4,4] matrix (numpy)."""
    return (ctypes.c_double * 12)(*[float(x) for x in m[:3].reshape(-1)])


def _cam4(cam):
    return (ctypes.c_double * 4)(float(cam['fx']), float(cam['fy']), float(cam['cx']), float(cam['cy']))


def tsdf_touch(depth, c2w, cam, stride, sdf_trunc, voxel_length, unit_lo, nu, stamp, stamps):
    """Stamp the units within sdf_trunc of the frame's sampled depth pixels (enslam_tsdf_touch).  depth float32 [H,W] on the
    HIP device, c2w float64 numpy [3|4,4], stamps int32 [nu0*nu1*nu2].  Returns the per-workgroup counts (int32 device
    tensor) of pixels that reached outside the table."""
    lib = L.lib()
    H, W = int(cam['H']), int(cam['W'])
    if depth.dtype is not torch.float32 or tuple(depth.shape) != (H, W) or not depth.is_contiguous():
        raise L.EnslamError(f"depth must be contiguous float32 [{H},{W}] (got {depth.dtype} {tuple(depth.shape)})")
    ns = -(-H // int(stride)) * -(-W // int(stride))
    outside = torch.empty(-(-ns // 256), dtype=torch.int32, device=depth.device)
    with torch.cuda.device(depth.device):
        L.check(lib.enslam_tsdf_touch(_ptr(depth), H, W, int(stride), _cam4(cam), _pose12(c2w), float(sdf_trunc),
                                      float(voxel_length), _i32x3(unit_lo), _i32x3(nu), int(stamp), _ptr(stamps), _ptr(outside),
                                      _stream()), "enslam_tsdf_touch")
    return outside


def tsdf_integrate(depth, color, mult, w2c, cam, voxel_length, sdf_trunc, unit_lo, nu, touched_block, touched_index, n_blocks,
                   tsdf, weight, vcolor):
    """Fuse one frame into the touched blocks (enslam_tsdf_integrate); returns the per-(block, slab) counts of updated voxels
    (int32 device tensor [n_touched * 16])."""
    lib = L.lib()
    H, W = int(cam['H']), int(cam['W'])
    n = int(touched_block.shape[0])
    counts = torch.empty(n * 16, dtype=torch.int32, device=depth.device)
    with torch.cuda.device(depth.device):
        L.check(lib.enslam_tsdf_integrate(_ptr(depth), _ptr(color), _ptr(mult), H, W, _cam4(cam), _pose12(w2c), float(voxel_length),
                                          float(sdf_trunc), _i32x3(unit_lo), _i32x3(nu), n, _ptr(touched_block), _ptr(touched_index),
                                          int(n_blocks), _ptr(tsdf), _ptr(weight), _ptr(vcolor), _ptr(counts), _stream()),
                "enslam_tsdf_integrate")
    return counts


def tsdf_mesh(table, unit_lo, nu, n_blocks, sorted_block, sorted_index, tsdf, weight, vcolor, voxel_length):
    """(vertices float64 [V,3], faces int32 [F,3], colors uint8 [V,3] or None) of the zero level of a block-sparse TSDF volume
    (enslam_tsdf_mesh_count / _emit; conventions: enslam_hip.h).  One host synchronisation: the counts."""
    lib = L.lib()
    dev = table.device
    with torch.cuda.device(dev):
        nbytes = ctypes.c_int64()
        L.check(lib.enslam_tsdf_mesh_workspace(int(n_blocks), ctypes.byref(nbytes)), "enslam_tsdf_mesh_workspace")
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        L.check(lib.enslam_tsdf_mesh_count(_ptr(table), _i32x3(nu), int(n_blocks), _ptr(sorted_block), _ptr(sorted_index),
                                           _ptr(tsdf), _ptr(weight), _ptr(ws), _ptr(counts), _stream()), "enslam_tsdf_mesh_count")
        n_verts, n_faces = counts.tolist()
        verts = torch.empty((n_verts, 3), dtype=torch.float64, device=dev)
        faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
        colors = torch.empty((n_verts, 3), dtype=torch.uint8, device=dev) if vcolor is not None else None
        L.check(lib.enslam_tsdf_mesh_emit(_ptr(table), _i32x3(unit_lo), _i32x3(nu), int(n_blocks), _ptr(sorted_block),
                                          _ptr(sorted_index), _ptr(tsdf), _ptr(weight), _ptr(vcolor), float(voxel_length), _ptr(ws),
                                          n_verts, n_faces, _ptr(verts) if n_verts else None, _ptr(faces) if n_faces else None,
                                          _ptr(colors) if colors is not None and n_verts else None, _stream()),
                "enslam_tsdf_mesh_emit")
    return verts, faces, colors


# ------------------------------------------------------------------------------------------------
# Frame preparation (csrc/frame_prep.hip): raw decoded images -> the tensors of the dataset readers
# ------------------------------------------------------------------------------------------------
EVENT_ORDERS = {'replica': (1, 2), 'rpg': (1, 0)}     # (channel of -, channel of +) in the event png: (0,-,+) / (+,-,0)


def frame_plan(color_shape, depth_shape, depth_int32, event_shape=None, K=None, distortion=None, png_depth_scale=1.0, scale=1.0,
               crop_size=None, crop_edge=0, event_order='replica', undistort_events=True):
    """The enslam_frame_plan of one frame layout (host arithmetic only; `frame_prepare` documents the arguments)."""
    if len(color_shape) == 2:
        color_shape = tuple(color_shape) + (1,)
    if len(color_shape) != 3 or len(depth_shape) != 2 or (event_shape is not None and (len(event_shape) != 3 or event_shape[2] != 3)):
        raise L.EnslamError(f"frame_prepare: colour must be [h,w] or [h,w,C], depth [H,W], events [h,w,3] (got {tuple(color_shape)}, "
                            f"{tuple(depth_shape)}, {None if event_shape is None else tuple(event_shape)})")
    if event_order not in EVENT_ORDERS:
        raise L.EnslamError(f"frame_prepare: event_order must be one of {sorted(EVENT_ORDERS)} (got {event_order!r})")
    p = L.FramePlan()
    p.h0, p.w0, p.channels = (int(v) for v in color_shape)
    p.he, p.we = (int(event_shape[0]), int(event_shape[1])) if event_shape is not None else (0, 0)
    p.H, p.W = int(depth_shape[0]), int(depth_shape[1])
    p.depth_int32 = int(bool(depth_int32))
    p.has_dist = int(distortion is not None)
    p.undistort_events = int(bool(undistort_events))
    if distortion is not None:
        if K is None:
            raise L.EnslamError("frame_prepare: a lens model needs the intrinsics K = (fx, fy, cx, cy)")
        p.fx, p.fy, p.cx, p.cy = (float(v) for v in K)
        d = [float(v) for v in distortion][:8]
        for i, v in enumerate(d):
            p.dist[i] = v
    p.crop_h, p.crop_w = (int(crop_size[0]), int(crop_size[1])) if crop_size is not None else (0, 0)
    p.crop_edge = int(crop_edge)
    p.ev_neg, p.ev_pos = EVENT_ORDERS[event_order]
    p.png_depth_scale, p.scale = float(png_depth_scale), float(scale)
    return p


def _raw_image(a, device, what, dtypes):
    """numpy array or tensor -> contiguous tensor on `device` (a numpy array is uploaded as it is: the raw bytes)."""
    if not torch.is_tensor(a):
        import numpy as np
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint16:                      # torch has no arithmetic on uint16: the bits travel as int16
            a = a.view(np.int16)
        a = torch.from_numpy(a)
    if a.dtype not in dtypes:
        raise L.EnslamError(f"frame_prepare: {what} must be one of {[str(d) for d in dtypes]} (got {a.dtype})")
    return a.to(device).contiguous()


def frame_prepare(color, depth, event=None, events=False, K=None, distortion=None, png_depth_scale=1.0, scale=1.0, crop_size=None,
                  crop_edge=0, event_order='replica', undistort_events=True, device=None):
    """One frame from raw decoded images to what the dataset readers hand out, in one launch (enslam_frame_prepare,
    enslam_hip.h): the device route of `datasets.BaseDataset` / `Replica_event` / `RPG_event`.

      color   uint8 [h0,w0,3], or grey [h0,w0] / [h0,w0,1] (replicated to three channels)
      depth   uint16 or int32 [H,W] (a tensor carries uint16 as the bits of an int16)
      event   uint8 [he,we,3] or None; `events=True` (implied by an event image) asks for the event outputs: without an
              image they are all zero (frame 0)
    numpy arrays are uploaded to `device` (default: the current HIP device), tensors must already live on a HIP device.
    K = (fx, fy, cx, cy) and distortion (k1, k2, p1, p2[, k3[, k4, k5, k6]]) remove the lens model from the colour image
    and, with undistort_events, from the event image -- never from the depth.  event_order: 'replica' for pngs with
    channels (0, -, +), 'rpg' for (+, -, 0).

    Returns (color float64 [H',W',3], depth float32 [H',W']) or, with events, (color, depth, event [H',W',2] = (-, +) --
    uint8 without crop_size, float32 with it --, mask int64 [H',W'])."""
    lib = L.lib()
    tensors = [t for t in (color, depth, event) if torch.is_tensor(t)]
    if device is None:
        device = tensors[0].device if tensors else torch.device('cuda', torch.cuda.current_device())
    device = torch.device(device)
    if device.type != 'cuda':
        raise L.EnslamError(f"frame_prepare runs on a HIP device (got {device}); the host route is datasets.BaseDataset with "
                            f"prepare='host'")
    for t in tensors:
        _require_hip(t, "frame_prepare: a raw image tensor")
    c = _raw_image(color, device, "colour", (torch.uint8,))
    d = _raw_image(depth, device, "depth", (torch.int16, torch.int32) + ((torch.uint16,) if hasattr(torch, 'uint16') else ()))
    e = _raw_image(event, device, "events", (torch.uint8,)) if event is not None else None
    plan = frame_plan(tuple(c.shape), tuple(d.shape), d.dtype is torch.int32, None if e is None else tuple(e.shape), K, distortion,
                      png_depth_scale, scale, crop_size, crop_edge, event_order, undistort_events)
    Hs, Ws = (plan.crop_h, plan.crop_w) if plan.crop_h > 0 else (plan.H, plan.W)
    Ho, Wo = max(Hs - 2 * plan.crop_edge, 0), max(Ws - 2 * plan.crop_edge, 0)
    want_events = events or e is not None
    with torch.cuda.device(device):
        color_out = torch.empty((Ho, Wo, 3), dtype=torch.float64, device=device)
        depth_out = torch.empty((Ho, Wo), dtype=torch.float32, device=device)
        event_out = mask_out = None
        if want_events:
            event_out = torch.empty((Ho, Wo, 2), dtype=torch.float32 if plan.crop_h > 0 else torch.uint8, device=device)
            mask_out = torch.empty((Ho, Wo), dtype=torch.int64, device=device)
        L.check(lib.enslam_frame_prepare(ctypes.byref(plan), _ptr(c), _ptr(d), _ptr(e), _ptr(color_out), _ptr(depth_out),
                                         _ptr(event_out), _ptr(mask_out), _stream()), "enslam_frame_prepare")
    if want_events:
        return color_out, depth_out, event_out, mask_out
    return color_out, depth_out


# ------------------------------------------------------------------------------------------------
# iMAP mode (configs/imap.yaml): the 256-wide decoder (csrc/imap_mlp.hip) and density compositing
# ------------------------------------------------------------------------------------------------
IMAP_WS_LIMIT_BYTES = 1 << 30     # the backward's workspace per launch; larger point sets run in chunks


def imap_params(dec):
    """the iMAP decoder's 11 parameter tensors in the order of the enslam_imap_* entries (_lib.IMAP_PARAM_NAMES)"""
    named = dict(dec.named_parameters())
    return [named[n] for n in L.IMAP_PARAM_NAMES]


def imap_chunk_points():
    """largest point count (a multiple of 64) whose backward workspace stays within IMAP_WS_LIMIT_BYTES"""
    lib = L.lib()
    per = lib.enslam_imap_workspace_floats(1 << 16) / float(1 << 16) * 4
    return max(64, int(IMAP_WS_LIMIT_BYTES / per) // 64 * 64)


def _imap_bound(bound, dtype):
    if bound is None:
        return None
    b = bound.detach().cpu() if torch.is_tensor(bound) else torch.as_tensor(bound)
    b = b.reshape(3, 2)
    # Renderer.eval_points compares the points with 0-dim float64 bound entries: torch evaluates that in the points'
    # dtype, so float32 points meet the bound rounded to float32
    if dtype != torch.float64:
        b = b.to(dtype)
    return (ctypes.c_double * 6)(*[float(x) for x in b.double().reshape(-1)])


def _imap_pack(ps):
    lib = L.lib()
    packed = torch.empty(lib.enslam_imap_packed_floats(), dtype=torch.float32, device=ps[0].device)
    pv = (ctypes.c_void_p * 11)(*[p.data_ptr() for p in ps])
    L.check(lib.enslam_imap_pack(pv, _ptr(packed), _stream()), "enslam_imap_pack")
    return packed


class _ImapMlpFn(torch.autograd.Function):
    """raw [P,4] of the iMAP decoder at points [P,3]; gradient to the points and to all 11 parameters."""

    @staticmethod
    def forward(ctx, pts, bound6_, *params):
        lib = L.lib()
        ps = [_f32c(p) for p in params]
        x = pts.detach().to(torch.float64).contiguous()
        P = x.shape[0]
        packed = _imap_pack(ps)
        raw = torch.empty((P, 4), dtype=torch.float32, device=pts.device)
        L.check(lib.enslam_imap_fwd(P, _ptr(x), _ptr(packed), bound6_, _ptr(raw), _stream()), "enslam_imap_fwd")
        ctx.keep = (x, packed, ps, bound6_, pts.dtype)
        return raw

    @staticmethod
    def backward(ctx, g_raw):
        lib = L.lib()
        x, packed, ps, bound6_, pdtype = ctx.keep
        P, dev = x.shape[0], x.device
        g = g_raw.detach().float().contiguous()
        grads = [torch.empty_like(p) for p in ps]
        d_pts = torch.empty((P, 3), dtype=torch.float32, device=dev)
        chunk = min(max(P, 1), imap_chunk_points())
        ws = torch.empty(lib.enslam_imap_workspace_floats(chunk), dtype=torch.float32, device=dev)
        pv = (ctypes.c_void_p * 11)(*[p.data_ptr() for p in ps])
        gv = (ctypes.c_void_p * 11)(*[t.data_ptr() for t in grads])
        for i, c0 in enumerate(range(0, max(P, 1), chunk)):
            n = min(chunk, P - c0)
            L.check(lib.enslam_imap_bwd(n, _ptr(x[c0:]) if n > 0 else None, pv, _ptr(packed), bound6_,
                                        _ptr(g[c0:]) if n > 0 else None, _ptr(ws), int(i > 0), gv,
                                        _ptr(d_pts[c0:]) if n > 0 else None, _stream()), "enslam_imap_bwd")
        return (d_pts.to(pdtype), None) + tuple(grads)


def imap_mlp(p, dec, bound=None):
    """raw [P,4] float32 of the iMAP decoder `dec` at points p [P,3] (float32 or float64; evaluated as float32 like the
    reference's p.float()).  With `bound`, points not strictly inside get sigma = 100 (Renderer.eval_points).
    Differentiable in p and in the decoder's parameters."""
    _require_hip(p, "points")
    ps = imap_params(dec)
    for t in ps:
        _require_hip(t, "decoder parameters")
    return _ImapMlpFn.apply(p.reshape(-1, 3), _imap_bound(bound, p.dtype), *ps)


class _CompositeDensityFn(torch.autograd.Function):
    """raw2outputs_nerf_color with occupancy=False as one HIP kernel each way; gradient to `raw` and `rays_d`."""

    @staticmethod
    def forward(ctx, raw, z_vals, rays_d):
        lib = L.lib()
        _require_hip(raw, "raw")
        N, S = z_vals.shape
        if S > 64:
            raise L.EnslamError("composite kernels handle at most 64 samples per ray")
        r = _f32c(raw)
        z = z_vals.detach().contiguous().double()
        d = _f32c(rays_d)
        dev = raw.device
        depth = torch.empty(N, dtype=torch.float64, device=dev)
        var = torch.empty(N, dtype=torch.float64, device=dev)
        rgb = torch.empty((N, 3), dtype=torch.float32, device=dev)
        w = torch.empty((N, S), dtype=torch.float32, device=dev)
        L.check(lib.enslam_composite_density_fwd(N, S, _ptr(r), _ptr(z), _ptr(d), _ptr(depth), _ptr(var), _ptr(rgb), _ptr(w),
                                                 _stream()), "enslam_composite_density_fwd")
        ctx.keep = (r, z, d, depth, rays_d.dtype)
        ctx.mark_non_differentiable(w)
        return depth, var, rgb, w

    @staticmethod
    def backward(ctx, g_depth, g_var, g_rgb, _gw):
        lib = L.lib()
        r, z, d, depth, ddtype = ctx.keep
        N, S = z.shape
        gD = g_depth.detach().double().contiguous() if g_depth is not None else None
        gV = g_var.detach().double().contiguous() if g_var is not None else None
        gC = g_rgb.detach().float().contiguous() if g_rgb is not None else None
        d_raw = torch.empty((N, S, 4), dtype=torch.float32, device=r.device)
        d_rd = torch.empty((N, 3), dtype=torch.float32, device=r.device)
        L.check(lib.enslam_composite_density_bwd(N, S, _ptr(r), _ptr(z), _ptr(d), _ptr(depth), _ptr(gD), _ptr(gV), _ptr(gC),
                                                 _ptr(d_raw), _ptr(d_rd), _stream()), "enslam_composite_density_bwd")
        return d_raw, None, d_rd.to(ddtype)


def composite_density(raw, z_vals, rays_d):
    """(depth f64 [N], var f64 [N], rgb f32 [N,3], weights f32 [N,S]) of raw [N,S,4] (sigma = volume density), z_vals
    [N,S], rays_d [N,3]: raw2outputs_nerf_color(occupancy=False)."""
    return _CompositeDensityFn.apply(raw, z_vals, rays_d)


# ------------------------------------------------------------------------------------------------
# event network (csrc/event_net.hip; event.compile_event_net is the public face)
# ------------------------------------------------------------------------------------------------
class EventNetWorkspace:
    """The device workspace of one image size: saved activations, gradient scratch, split-reduction partials.  `generation`
    counts the forwards that have written it, so a backward can tell whether it still holds ITS forward."""

    def __init__(self, H, W, device):
        n = L.lib().enslam_eventnet_workspace_floats(H, W)
        if n == 0:
            raise L.EnslamError(f"event network: unsupported image size {H} x {W}")
        self.H, self.W = H, W
        self.buf = torch.empty(n, dtype=torch.float32, device=device)
        self.generation = 0


# Calls made so far (tests read it):
#   'wgrad'        backward passes that ran the convolutions' weight gradients;
#   'heads_wgrad'  backward passes that built the heads block's gradient alone;
#   'fold_pack'    packed images built on the device from live parameters;
#   'train_forward' / 'train_backward'  whole-net calls of the training-mode BatchNorm route, 'bn_running' its running-
#                  statistics updates; 'bn_stats' / 'bn_apply' / 'bn_backward' the single-operation entries.
eventnet_launches = {'forward': 0, 'backward': 0, 'wgrad': 0, 'heads_wgrad': 0, 'fold_pack': 0, 'train_forward': 0,
                     'train_backward': 0, 'bn_running': 0, 'bn_stats': 0, 'bn_apply': 0, 'bn_backward': 0}


def eventnet_forward(packed, x, ws):
    """x float32 contiguous [1,6,H,W] -> (events, probs) [1,2,H,W]; leaves the activations in `ws`."""
    events = torch.empty((1, 2, ws.H, ws.W), dtype=torch.float32, device=x.device)
    probs = torch.empty_like(events)
    L.check(L.lib().enslam_eventnet_forward(_ptr(packed), _ptr(x), ws.H, ws.W, _ptr(ws.buf), _ptr(events), _ptr(probs),
                                            _stream()), "enslam_eventnet_forward")
    ws.generation += 1
    eventnet_launches['forward'] += 1
    return events, probs


def eventnet_backward(packed, ws, g_events, g_probs):
    g_x = torch.empty((1, 6, ws.H, ws.W), dtype=torch.float32, device=g_events.device)
    L.check(L.lib().enslam_eventnet_backward(_ptr(packed), _ptr(ws.buf), _ptr(g_events), _ptr(g_probs), _ptr(g_x), ws.H, ws.W,
                                             _stream()), "enslam_eventnet_backward")
    eventnet_launches['backward'] += 1
    return g_x


class _EventNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, packed, ws):
        xc = _f32c(x)
        events, probs = eventnet_forward(packed, xc, ws)
        ctx.packed, ctx.ws, ctx.generation = packed, ws, ws.generation
        ctx.save_for_backward(xc)
        return events, probs

    @staticmethod
    def backward(ctx, g_events, g_probs):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        ws = ctx.ws
        if ws.generation != ctx.generation:              # another forward of this size ran in between: restore the activations
            eventnet_forward(ctx.packed, ctx.saved_tensors[0], ws)
        return eventnet_backward(ctx.packed, ws, _f32c(g_events), _f32c(g_probs)), None, None


def eventnet_apply(x, packed, ws):
    _require_hip(x, "the event network's input")
    return _EventNetFn.apply(x, packed, ws)


class EventNetTrainScratch:
    """Split partials of the weight gradients of one image size (enslam_eventnet_wgrad_scratch_floats)."""

    def __init__(self, H, W, device):
        n = L.lib().enslam_eventnet_wgrad_scratch_floats(H, W)
        if n == 0:
            raise L.EnslamError(f"event network: unsupported image size {H} x {W}")
        self.buf = torch.empty(n, dtype=torch.float32, device=device)


def eventnet_backward_weights(packed, ws, scratch, g_events, g_probs, want_gx=True):
    """(g_x or None, g_packed): the input gradient and the gradient of the packed image (Wt blocks and pad zero)."""
    g_x = torch.empty((1, 6, ws.H, ws.W), dtype=torch.float32, device=g_events.device) if want_gx else None
    g_packed = torch.empty_like(packed)
    L.check(L.lib().enslam_eventnet_backward_weights(_ptr(packed), _ptr(ws.buf), _ptr(g_events), _ptr(g_probs), _ptr(g_x),
                                                     _ptr(g_packed), _ptr(scratch.buf), scratch.buf.numel(), ws.H, ws.W,
                                                     _stream()), "enslam_eventnet_backward_weights")
    eventnet_launches['backward'] += 1
    eventnet_launches['wgrad'] += 1
    return g_x, g_packed


def eventnet_heads_wgrad(packed, ws, scratch, g_events, g_probs):
    """g_packed with only the heads block's gradient built; everything else zero."""
    g_packed = torch.zeros_like(packed)
    heads = g_packed[-264:]
    L.check(L.lib().enslam_eventnet_heads_wgrad(_ptr(ws.buf), _ptr(g_events), _ptr(g_probs), _ptr(heads), _ptr(scratch.buf),
                                                scratch.buf.numel(), ws.H, ws.W, _stream()), "enslam_eventnet_heads_wgrad")
    eventnet_launches['heads_wgrad'] += 1
    return g_packed


class _EventNetTrainFn(torch.autograd.Function):
    """_EventNetFn with the packed image as a second differentiable input."""

    @staticmethod
    def forward(ctx, x, packed, ws, scratch, convs_hot):
        xc, pc = _f32c(x), _f32c(packed)
        events, probs = eventnet_forward(pc, xc, ws)
        ctx.ws, ctx.scratch, ctx.generation, ctx.convs_hot = ws, scratch, ws.generation, convs_hot
        ctx.save_for_backward(xc, pc)
        return events, probs

    @staticmethod
    def backward(ctx, g_events, g_probs):
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_w):
            return None, None, None, None, None
        if _capturing():
            raise RuntimeError("the trainable HIP event network does not support graph capture of a training step")
        xc, pc = ctx.saved_tensors
        ws = ctx.ws
        if ws.generation != ctx.generation:              # another forward of this size ran in between: restore the activations
            eventnet_forward(pc, xc, ws)
        ge, gp = _f32c(g_events), _f32c(g_probs)
        if need_w and ctx.convs_hot:
            g_x, g_packed = eventnet_backward_weights(pc, ws, ctx.scratch, ge, gp, want_gx=need_x)
            return g_x, g_packed, None, None, None
        g_x = eventnet_backward(pc, ws, ge, gp) if need_x else None
        g_packed = eventnet_heads_wgrad(pc, ws, ctx.scratch, ge, gp) if need_w else None
        return g_x, g_packed, None, None, None


def eventnet_train_apply(x, packed, ws, scratch, convs_hot=True):
    """(events, probs) of x [1,6,H,W] and the packed image, differentiable in both.  `convs_hot` False: only the heads
    block of the packed image's gradient is wanted (no convolution weight gradient is launched)."""
    _require_hip(x, "the event network's input")
    _require_hip(packed, "the event network's packed weights")
    return _EventNetTrainFn.apply(x, packed, ws, scratch, convs_hot)


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


_fold_scratch = {}                      # device -> float64 [26 * 16384], the partial sums of fold_pack_backward


def _fold_flat(consts, params):
    """The address order of enslam_eventnet_fold_pack: per convolution w, gamma, beta, sq, shift; then the heads' four."""
    flat = []
    for i in range(26):
        flat += [params[3 * i], params[3 * i + 1], params[3 * i + 2], consts[2 * i], consts[2 * i + 1]]
    return flat + list(params[78:])


class _EventNetFoldPackFn(torch.autograd.Function):
    """The packed image from live parameters (enslam_eventnet_fold_pack) and its chain rule back to them.  Inputs: the 52
    float64 constants (sq, shift per convolution; no gradient), then per convolution w, gamma, beta and the heads' four.
    All of them are saved through save_for_backward, so a parameter updated in place between forward and backward is an
    autograd error, not a gradient from other weights."""

    @staticmethod
    def forward(ctx, n_const, *tensors):
        consts, params = tensors[:n_const], tensors[n_const:]
        packed = torch.empty(L.lib().enslam_eventnet_pack_floats(), dtype=torch.float32, device=params[0].device)
        L.check(L.lib().enslam_eventnet_fold_pack(_ptr_array(_fold_flat(consts, params)), _ptr(packed), _stream()),
                "enslam_eventnet_fold_pack")
        eventnet_launches['fold_pack'] += 1
        ctx.n_const = n_const
        ctx.save_for_backward(*tensors)
        return packed

    @staticmethod
    def backward(ctx, g_packed):
        n_const = ctx.n_const
        tensors = ctx.saved_tensors
        consts, params = tensors[:n_const], tensors[n_const:]
        needs = ctx.needs_input_grad[1 + n_const:]
        g = _f32c(g_packed)
        none = (None,) * (1 + n_const)
        if not any(needs[:78]):                                    # the heads alone: their gradients are slices of the block
            h = g[-264:]
            heads = (h[:128].view(params[78].shape), h[128:256].view(params[79].shape), h[256:258], h[258:260])
            return none + (None,) * 78 + tuple(t if need else None for t, need in zip(heads, needs[78:]))
        sizes = [p.numel() for p in params]
        buf = torch.empty(sum(sizes), dtype=torch.float32, device=g.device)      # one allocation, the gradients are its views
        grads = [t.view(p.shape) for t, p in zip(buf.split(sizes), params)]
        base, at, addr = buf.data_ptr(), 0, []
        for n in sizes:
            addr.append(base + 4 * at)
            at += n
        scratch = _fold_scratch.get(g.device)
        if scratch is None:
            scratch = _fold_scratch[g.device] = torch.empty(26 * 16384, dtype=torch.float64, device=g.device)
        L.check(L.lib().enslam_eventnet_fold_pack_backward(_ptr_array(_fold_flat(consts, params)), _ptr(g),
                                                           (ctypes.c_void_p * len(addr))(*addr), _ptr(scratch), _stream()),
                "enslam_eventnet_fold_pack_backward")
        return none + tuple(t if need else None for t, need in zip(grads, needs))


def eventnet_fold_pack(params, consts):
    """params: [w, gamma, beta] x 26 + [W1, W2, b1, b2], float32 contiguous on the device; consts: [sq, shift] x 26, float64 on
    the device.  The packed image, differentiable in the parameters."""
    return _EventNetFoldPackFn.apply(len(consts), *consts, *params)


# training-mode BatchNorm and batches (enslam_eventnet_bn_* / enslam_eventnet_train_*; event.compile_event_net_batchnorm)
EVENTNET_BN_COUT = tuple(cout for _, cout in EVENTNET_CONVS)       # one BatchNorm per convolution, in packing order
EVENTNET_BN_CHANNELS = sum(EVENTNET_BN_COUT)         # 5888: the length of the concatenated batch statistics
EVENTNET_BN_ROWS = 256                               # rows per chunk of the BatchNorm kernels (BN_ROWS of csrc/event_net.hip)


def eventnet_conv_level(i):
    """The resolution level (0 = full size) of convolution i in packing order."""
    return i // 2 if i < 10 else 3 - ((i - 10) % 8) // 2


def _bn_scratch(M, C, device, backward=False):
    chunks = (M + EVENTNET_BN_ROWS - 1) // EVENTNET_BN_ROWS
    return torch.empty(2 * chunks * C + (2 * C if backward else 0), dtype=torch.float64, device=device)


def eventnet_bn_stats(z):
    """(mean, var) float64 [C] of z float32 [M, C]: the batch mean and the biased variance."""
    _require_hip(z, "the BatchNorm input")
    z = _f32c(z)
    M, C = z.shape
    mean = torch.empty(C, dtype=torch.float64, device=z.device)
    var = torch.empty_like(mean)
    scratch = _bn_scratch(M, C, z.device)
    L.check(L.lib().enslam_eventnet_bn_stats(_ptr(z), M, C, _ptr(mean), _ptr(var), _ptr(scratch), scratch.numel(), _stream()),
            "enslam_eventnet_bn_stats")
    eventnet_launches['bn_stats'] += 1
    return mean, var


def eventnet_bn_apply(z, gamma, beta, mean, var, eps, relu=True):
    """y float32 [M, C] = relu(gamma (z - mean) / sqrt(var + eps) + beta) with float64 mean / var [C]."""
    _require_hip(z, "the BatchNorm input")
    z = _f32c(z)
    M, C = z.shape
    y = torch.empty_like(z)
    L.check(L.lib().enslam_eventnet_bn_apply(_ptr(z), _ptr(_f32c(gamma)), _ptr(_f32c(beta)), _ptr(mean), _ptr(var), float(eps), M,
                                             C, int(bool(relu)), _ptr(y), _stream()), "enslam_eventnet_bn_apply")
    eventnet_launches['bn_apply'] += 1
    return y


def eventnet_bn_backward(z, y, g_y, gamma, mean, var, eps):
    """(g_z [M, C], dgamma [C], dbeta [C]) float32 of BatchNorm (+ ReLU where y, its output, is given; y None: no ReLU)."""
    _require_hip(z, "the BatchNorm input")
    z, g_y = _f32c(z), _f32c(g_y)
    y = _f32c(y) if y is not None else None
    M, C = z.shape
    g_z = torch.empty_like(z)
    dgamma = torch.empty(C, dtype=torch.float32, device=z.device)
    dbeta = torch.empty_like(dgamma)
    scratch = _bn_scratch(M, C, z.device, backward=True)
    L.check(L.lib().enslam_eventnet_bn_backward(_ptr(z), _ptr(y), _ptr(g_y), _ptr(_f32c(gamma)), _ptr(mean), _ptr(var),
                                                float(eps), M, C, _ptr(g_z), _ptr(dgamma), _ptr(dbeta), _ptr(scratch),
                                                scratch.numel(), _stream()), "enslam_eventnet_bn_backward")
    eventnet_launches['bn_backward'] += 1
    return g_z, dgamma, dbeta


def eventnet_bn_running(buffers, batch_mean, batch_var, B, H, W, momentum):
    """In place on `buffers` ([running_mean, running_var] x 26, float32 on the device): torch's running-statistics rule with
    the batch statistics float64 [5888] of a training-mode forward of a [B,6,H,W] input."""
    L.check(L.lib().enslam_eventnet_bn_running(_ptr_array(buffers), _ptr(batch_mean), _ptr(batch_var), B, H, W, float(momentum),
                                               _stream()), "enslam_eventnet_bn_running")
    eventnet_launches['bn_running'] += 1


class EventNetBnWorkspace:
    """The device workspace of the training-mode route for one input size [B,6,H,W]: per convolution the raw output and the
    BatchNorm + ReLU output, the packed weights, the batch statistics, gradient and reduction scratch.  `generation` counts
    the forwards that have written it, so a backward can tell whether it still holds ITS forward."""

    def __init__(self, B, H, W, device):
        n = L.lib().enslam_eventnet_bn_workspace_floats(B, H, W)
        if n == 0:
            raise L.EnslamError(f"event network (training mode): unsupported input size {B} x {H} x {W}")
        self.B, self.H, self.W = B, H, W
        self.buf = torch.empty(n, dtype=torch.float32, device=device)
        self.batch_mean = torch.empty(EVENTNET_BN_CHANNELS, dtype=torch.float64, device=device)
        self.batch_var = torch.empty_like(self.batch_mean)
        self.generation = 0

    def saved(self, i):
        """Read-only view [B, H_i, W_i, C_i] of convolution i's post-ReLU output from the last forward."""
        if not 0 <= i < 26:
            raise IndexError(f"the event network has 26 convolutions (got {i})")
        at = L.lib().enslam_eventnet_bn_saved_offset(self.B, self.H, self.W, i)
        lvl, C = eventnet_conv_level(i), EVENTNET_BN_COUT[i]
        h, w = self.H >> lvl, self.W >> lvl
        return self.buf[at:at + self.B * h * w * C].view(self.B, h, w, C).detach()


def eventnet_train_forward(params, x, ws, eps):
    """x float32 contiguous [B,6,H,W] -> (events, probs) [B,2,H,W] of the training-mode net; leaves the activations and the
    batch statistics in `ws`.  params: [w, gamma, beta] x 26 + [W1, W2, b1, b2], float32 contiguous on the device."""
    events = torch.empty((ws.B, 2, ws.H, ws.W), dtype=torch.float32, device=x.device)
    probs = torch.empty_like(events)
    L.check(L.lib().enslam_eventnet_train_forward(_ptr_array(params), _ptr(x), ws.B, ws.H, ws.W, float(eps), _ptr(ws.buf),
                                                  _ptr(events), _ptr(probs), _ptr(ws.batch_mean), _ptr(ws.batch_var), _stream()),
            "enslam_eventnet_train_forward")
    ws.generation += 1
    eventnet_launches['train_forward'] += 1
    return events, probs


def eventnet_train_backward(params, ws, g_events, g_probs, eps, needs, want_gx=True):
    """(g_x or None, [gradient or None per parameter]): `needs` says which of the 82 parameters want one.  The gradients are
    views of one allocation; a convolution weight that wants none costs no weight-gradient launch."""
    dev = g_events.device
    g_x = torch.empty((ws.B, 6, ws.H, ws.W), dtype=torch.float32, device=dev) if want_gx else None
    needs = list(needs)
    alloc = needs[:78] + [any(needs[78:])] * 4           # the heads' four come together
    sizes = [p.numel() if a else 0 for p, a in zip(params, alloc)]
    buf = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
    base, at, addr, grads = buf.data_ptr(), 0, [], []
    for p, n, a in zip(params, sizes, alloc):
        addr.append(base + 4 * at if a else None)
        grads.append(buf[at:at + n].view(p.shape) if a else None)
        at += n
    L.check(L.lib().enslam_eventnet_train_backward(_ptr_array(params), _ptr(ws.buf), _ptr(g_events), _ptr(g_probs), ws.B, ws.H,
                                                   ws.W, float(eps), _ptr(g_x), (ctypes.c_void_p * len(addr))(*addr), _stream()),
            "enslam_eventnet_train_backward")
    eventnet_launches['train_backward'] += 1
    return g_x, [g if need else None for g, need in zip(grads, needs)]


class _EventNetBnFn(torch.autograd.Function):
    """The whole training-mode net: inputs x and the 82 parameters, differentiable in all of them.  With `buffers` (the 52
    running statistics) the forward also applies torch's running-statistics rule to them, in place."""

    @staticmethod
    def forward(ctx, x, ws, eps, momentum, buffers, *params):
        xc = _f32c(x)
        pc = [p.detach() for p in params]
        events, probs = eventnet_train_forward(pc, xc, ws, eps)
        if buffers is not None:
            eventnet_bn_running(buffers, ws.batch_mean, ws.batch_var, ws.B, ws.H, ws.W, momentum)
        ctx.ws, ctx.eps, ctx.generation = ws, eps, ws.generation
        ctx.save_for_backward(xc, *params)
        return events, probs

    @staticmethod
    def backward(ctx, g_events, g_probs):
        need_x, needs = ctx.needs_input_grad[0], ctx.needs_input_grad[5:]
        if not (need_x or any(needs)):
            return (None,) * (5 + len(needs))
        if _capturing():
            raise NotImplementedError("the training-mode HIP event network does not support graph capture of a training step")
        xc, pc = ctx.saved_tensors[0], [p.detach() for p in ctx.saved_tensors[1:]]
        ws = ctx.ws
        if ws.generation != ctx.generation:              # another forward of this size ran in between: restore the activations
            eventnet_train_forward(pc, xc, ws, ctx.eps)
        g_x, grads = eventnet_train_backward(pc, ws, _f32c(g_events), _f32c(g_probs), ctx.eps, needs, want_gx=need_x)
        return (g_x, None, None, None, None) + tuple(grads)


def eventnet_bn_net_apply(x, params, ws, eps, momentum, buffers):
    """(events, probs) [B,2,H,W] of x [B,6,H,W] through the training-mode net on the device: batch statistics in the forward,
    their terms in the backward.  params: [w, gamma, beta] x 26 + [W1, W2, b1, b2], contiguous float32 on the device;
    buffers: [running_mean, running_var] x 26 updated in place with `momentum`, or None to leave them alone."""
    _require_hip(x, "the event network's input")
    return _EventNetBnFn.apply(x, ws, eps, momentum, buffers, *params)


# ------------------------------------------------------------------------------------------------
# Event-camera simulator (csrc/event_sim.hip; event_sim.EventSimulator drives it)
# ------------------------------------------------------------------------------------------------
def event_sim_plan(H, W, substeps, eps, c_pos, c_neg, channels=1, init=False, cam=None, room=None):
    """The enslam_event_sim_plan of one launch (host arithmetic only).  cam: dict with fx, fy, cx, cy and room: a
    synthetic.BoxRoom, both for the analytic route only."""
    p = L.EventSimPlan()
    p.H, p.W, p.K, p.channels, p.init = int(H), int(W), int(substeps), int(channels), int(bool(init))
    p.eps, p.c_pos, p.c_neg = float(eps), float(c_pos), float(c_neg)
    if cam is not None:
        p.fx, p.fy, p.cx, p.cy = (float(cam[k]) for k in ('fx', 'fy', 'cx', 'cy'))
    if room is not None:
        p.room_lo[:], p.room_hi[:] = room.room_lo.tolist(), room.room_hi.tolist()
        p.has_box = int(room.box_lo is not None)
        if p.has_box:
            p.box_lo[:], p.box_hi[:] = room.box_lo.tolist(), room.box_hi.tolist()
        p.freq[:], p.phase[:] = room.freq.reshape(-1).tolist(), room.phase.tolist()
    return p


def _event_sim_checks(what, H, W, substeps, eps, c_pos, c_neg, state, c_pos_map, c_neg_map, init):
    if H <= 0 or W <= 0:
        raise L.EnslamError(f"{what}: the image must have pixels (got {H} x {W})")
    kmax = L.lib().enslam_event_sim_max_substeps()
    if not 1 <= int(substeps) <= kmax:
        raise L.EnslamError(f"{what}: substeps must be in 1..{kmax} (got {substeps})")
    if not (eps > 0 and eps < float('inf')):
        raise L.EnslamError(f"{what}: eps must be positive and finite (got {eps})")
    _event_sim_tensor(what, 'state', state, torch.float64, (H, W), None)
    for name, c, m in (('c_pos', c_pos, c_pos_map), ('c_neg', c_neg, c_neg_map)):
        if m is None:
            if not init and not (c > 0 and c < float('inf')):
                raise L.EnslamError(f"{what}: {name} must be positive and finite (got {c})")
        else:
            _event_sim_tensor(what, name + '_map', m, torch.float64, (H, W), state.device)


def _event_sim_tensor(what, name, t, dtype, shape, device):
    if not torch.is_tensor(t):
        raise L.EnslamError(f"{what}: {name} must be a tensor (got {type(t).__name__})")
    _require_hip(t, f"{what}: {name}")
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or (device is not None and t.device != device):
        raise L.EnslamError(f"{what}: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)}"
                            f"{'' if device is None else f' on {device}'} (got {t.dtype} {tuple(t.shape)} on {t.device}, "
                            f"contiguous: {t.is_contiguous()})")


def _event_image_source(what, prev, cur, state, stamps, substeps, eps, c_pos, c_neg, c_pos_map, c_neg_map, lut, levels, init):
    """Validates the images source of one interval (stamps None: the frame entry, which has none) and returns (H, W, stamps,
    src): src the arguments the three *_images entries share, from the plan to L_ref."""
    if not torch.is_tensor(state):
        raise L.EnslamError(f"{what}: state must be a tensor")
    H, W = (int(v) for v in state.shape) if state.dim() == 2 else (0, 0)
    _event_sim_checks(what, H, W, substeps, eps, c_pos, c_neg, state, c_pos_map, c_neg_map, init)
    if stamps is not None:
        stamps = _event_stamps(what, stamps)
    dev = state.device
    channels = 1
    if levels is not None:
        if len(levels) != 2:
            raise L.EnslamError(f"{what}: levels must be the pair (L_prev, L_cur)")
        for name, t in zip(('L_prev', 'L_cur'), levels):
            _event_sim_tensor(what, name, t, torch.float64, (H, W), dev)
        prev = cur = None
    else:
        if not torch.is_tensor(prev) or not torch.is_tensor(cur):
            raise L.EnslamError(f"{what}: prev and cur must be tensors (or pass `levels`)")
        for name, t in (('prev', prev), ('cur', cur)):
            if t.dim() not in (2, 3) or t.shape != cur.shape:
                raise L.EnslamError(f"{what}: prev and cur must be uint8 tensors of one shape [H,W] or [H,W,C]")
            shape = (H, W) if t.dim() == 2 else (H, W, int(t.shape[2]))
            if t.dim() == 3 and shape[2] not in (1, 3):
                raise L.EnslamError(f"{what}: images must have 1 or 3 channels (got {shape[2]})")
            _event_sim_tensor(what, name, t, torch.uint8, shape, dev)
        channels = 3 if cur.dim() == 3 and cur.shape[2] == 3 else 1
        if channels == 1:
            if lut is None:
                raise L.EnslamError(f"{what}: grey images need the host-computed table `lut` (float64 [256])")
            _event_sim_tensor(what, 'lut', lut, torch.float64, (256,), dev)
    plan = event_sim_plan(H, W, substeps, eps, c_pos, c_neg, channels=channels, init=init)
    la, lb = levels if levels is not None else (None, None)
    return H, W, stamps, (ctypes.byref(plan), _ptr(prev), _ptr(cur), _ptr(lut), _ptr(la), _ptr(lb), _ptr(c_pos_map),
                          _ptr(c_neg_map), _ptr(state))


def _event_room_source(what, room, poses, cam, state, stamps, eps, c_pos, c_neg, c_pos_map, c_neg_map, with_prev, init):
    """Validates the analytic source of one interval (stamps None: the frame entry; with_prev: row 0 of `poses` is the previous
    frame's) and returns (H, W, K, stamps, rows, src): rows the poses float64 [K(+1),3,4] on the device, which the caller keeps
    alive across its launches, and src the arguments the three *_boxroom entries share, from the plan to L_ref."""
    if not torch.is_tensor(state):
        raise L.EnslamError(f"{what}: state must be a tensor")
    H, W = int(cam['H']), int(cam['W'])
    p = poses if torch.is_tensor(poses) else torch.as_tensor(poses)
    if p.dim() != 3 or (with_prev and p.shape[0] < 2) or p.shape[1] not in (3, 4) or p.shape[2] != 4 or p.dtype != torch.float64:
        want = "[K+1,3|4,4], the previous frame's first" if with_prev else "[K,3|4,4]"
        raise L.EnslamError(f"{what}: poses must be float64 {want} (got {p.dtype} {tuple(p.shape)})")
    K = int(p.shape[0]) - int(with_prev)
    _event_sim_checks(what, H, W, K, eps, c_pos, c_neg, state, c_pos_map, c_neg_map, init)
    if stamps is not None:
        stamps = _event_stamps(what, stamps)
    if torch.is_tensor(poses):
        _require_hip(poses, f"{what}: a pose tensor")
    if not (float(cam['fx']) != 0 and float(cam['fy']) != 0):
        raise L.EnslamError(f"{what}: fx and fy must not be zero")
    rows = p[:, :3, :].to(state.device).contiguous()
    plan = event_sim_plan(H, W, K, eps, c_pos, c_neg, init=init, cam=cam, room=room)
    return H, W, K, stamps, rows, (ctypes.byref(plan), _ptr(rows), _ptr(c_pos_map), _ptr(c_neg_map), _ptr(state))


def event_sim_images(prev, cur, state, substeps=8, eps=1e-3, c_pos=0.2, c_neg=0.2, lut=None, levels=None, c_pos_map=None,
                     c_neg_map=None, init=False):
    """One interval of the image route (enslam_event_sim_images, enslam_hip.h): events uint8 [H,W,2] = (-, +) between two
    decoded images, `state` (L_ref, float64 [H,W] on a HIP device) updated in place.

      prev, cur  uint8 [H,W] / [H,W,1] (grey) or [H,W,3] (RGB) on the state's device
      lut        float64 [256]: log(v / 255 + eps) of the grey values, computed by the host (required for grey images)
      levels     (L_prev, L_cur) float64 [H,W]: host-computed log intensities used INSTEAD of the images (prev and cur may
                 then be None), so that no device log decides a count
      c_pos_map, c_neg_map  float64 [H,W] per-pixel thresholds replacing the scalars
      init       the first frame: no events (None is returned), state := L of `cur`"""
    H, W, _, src = _event_image_source("event_sim_images", prev, cur, state, None, substeps, eps, c_pos, c_neg, c_pos_map,
                                       c_neg_map, lut, levels, init)
    dev = state.device
    with torch.cuda.device(dev):
        events = None if init else torch.empty((H, W, 2), dtype=torch.uint8, device=dev)
        L.check(L.lib().enslam_event_sim_images(*src, _ptr(events), _stream()), "enslam_event_sim_images")
    return events


def event_sim_boxroom(room, poses, cam, state, eps=1e-3, c_pos=0.2, c_neg=0.2, c_pos_map=None, c_neg_map=None, init=False,
                      want_frame=False):
    """One interval of the analytic route (enslam_event_sim_boxroom, enslam_hip.h): the kernel renders synthetic.BoxRoom
    `room` at the K poses `poses` (float64 [K,3|4,4] camera-to-world on the state's device, or a host array that is uploaded;
    the last one is the frame the interval ends at) for the camera `cam` (H, W, fx, fy, cx, cy) and returns the events uint8
    [H,W,2] = (-, +); `state` (L_ref, float64 [H,W]) is updated in place.  want_frame: also (color float64 [H,W,3], depth
    float32 [H,W]) of the last pose, what BoxRoom.render returns.  init: the first frame -- no events (None), state := L."""
    H, W, _, _, rows, src = _event_room_source("event_sim_boxroom", room, poses, cam, state, None, eps, c_pos, c_neg, c_pos_map,
                                               c_neg_map, False, init)
    dev = state.device
    with torch.cuda.device(dev):
        events = None if init else torch.empty((H, W, 2), dtype=torch.uint8, device=dev)
        color = torch.empty((H, W, 3), dtype=torch.float64, device=dev) if want_frame else None
        depth = torch.empty((H, W), dtype=torch.float32, device=dev) if want_frame else None
        L.check(L.lib().enslam_event_sim_boxroom(*src, _ptr(events), _ptr(color), _ptr(depth), _stream()), "enslam_event_sim_boxroom")
    return (events, color, depth) if want_frame else events


# ------------------------------------------------------------------------------------------------
# Time-stamped event streams (csrc/event_stream.hip; event_sim.EventSimulator and event_stream.accumulate drive it)
# ------------------------------------------------------------------------------------------------
EVENT_ACCUMULATE_MAX_CELLS = 1 << 25        # B * H * W of one enslam_event_accumulate call (256 MiB of uint32 counts)


def _event_stamps(what, stamps):
    try:
        t_a, t_b = (float(v) for v in stamps)
    except (TypeError, ValueError):
        raise L.EnslamError(f"{what}: stamps must be the pair (t_a, t_b) of the interval's frame times") from None
    if not (t_a <= t_b and abs(t_a) < float('inf') and abs(t_b) < float('inf')):
        raise L.EnslamError(f"{what}: stamps must be finite with t_a <= t_b (got {t_a}, {t_b})")
    return t_a, t_b


def _event_stream_run(what, route, src, state, H, W, stamps, count_src=None, noise=None, t_last=None, stream=True):
    """The launches of one interval with time stamps on `route` ('images' / 'boxroom') from the source arguments `src`
    (`count_src`: what the count entry takes instead).  noise None: enslam_event_stream_*; otherwise the enslam_event_noise of
    the interval, for enslam_event_noisy_* with `t_last`.  stream: count -> prefix sum -> one read-back of the total -> emit,
    returns (events, (t, x, y, p)); otherwise (the noisy sensor only) the one launch of the count-image-only form, returns
    events."""
    if H > 65536 or W > 65536:
        raise L.EnslamError(f"{what}: event coordinates are uint16, the sensor is {H} x {W}")
    count_tail, emit_tail = (), ()
    if noise is not None:
        _event_sim_tensor(what, 't_last', t_last, torch.float64, (H, W), state.device)
        count_tail, emit_tail = (ctypes.byref(noise), *stamps, _ptr(t_last)), (ctypes.byref(noise), _ptr(t_last))
    lib, family = L.lib(), f"enslam_event_{'stream' if noise is None else 'noisy'}_{route}_"
    emit = getattr(lib, family + 'emit')
    dev = state.device
    with torch.cuda.device(dev):
        events = torch.empty((H, W, 2), dtype=torch.uint8, device=dev)
        if not stream:
            L.check(emit(*src, _ptr(events), None, 0, *stamps, None, None, None, None, *emit_tail, _stream()), what + " (image)")
            return events
        counts = torch.empty((H, W), dtype=torch.int64, device=dev)
        L.check(getattr(lib, family + 'count')(*(count_src or src), _ptr(counts), *count_tail, _stream()), what + " (count)")
        ends = torch.cumsum(counts.view(-1), 0)
        total = int(ends[-1].item())                            # the one read-back of the interval
        if total > 2 ** 31 - 1:
            raise L.EnslamError(f"{what}: {total} events in one interval (at most 2^31 - 1)")
        t = torch.empty(total, dtype=torch.float64, device=dev)
        x, y = (torch.empty(total, dtype=torch.uint16, device=dev) for _ in range(2))
        p = torch.empty(total, dtype=torch.uint8, device=dev)
        L.check(emit(*src, _ptr(events), _ptr(ends), total, *stamps, _ptr(t), _ptr(x), _ptr(y), _ptr(p), *emit_tail, _stream()),
                what + " (emit)")
    return events, (t, x, y, p)


def event_stream_images(prev, cur, state, stamps, substeps=8, eps=1e-3, c_pos=0.2, c_neg=0.2, lut=None, levels=None,
                        c_pos_map=None, c_neg_map=None):
    """One interval of the image route with time stamps (enslam_event_stream_images_*, enslam_hip.h): the arguments of
    `event_sim_images` plus stamps = (t_a, t_b), the times of the two frames.  Returns (events, (t, x, y, p)): the uint8
    [H,W,2] image `event_sim_images` returns (and the same update of `state`), and the events as device tensors -- t float64,
    x, y uint16, p uint8 (1 = positive) -- in pixel-major order, time-ordered within a pixel."""
    what = "event_stream_images"
    H, W, stamps, src = _event_image_source(what, prev, cur, state, stamps, substeps, eps, c_pos, c_neg, c_pos_map, c_neg_map, lut,
                                            levels, False)
    return _event_stream_run(what, 'images', src, state, H, W, stamps)


def event_stream_boxroom(room, poses, cam, state, stamps, eps=1e-3, c_pos=0.2, c_neg=0.2, c_pos_map=None, c_neg_map=None):
    """One interval of the analytic route with time stamps (enslam_event_stream_boxroom_*, enslam_hip.h).  poses: float64
    [K+1,3|4,4] -- row 0 the PREVIOUS frame's pose (rendered for the level the first sub-step starts from), rows 1..K the
    sub-steps, the last one the frame the interval ends at; stamps = (t_a, t_b).  Returns (events, (t, x, y, p)) as
    `event_stream_images`; `state` is updated as `event_sim_boxroom` updates it."""
    what = "event_stream_boxroom"
    H, W, _, stamps, rows, src = _event_room_source(what, room, poses, cam, state, stamps, eps, c_pos, c_neg, c_pos_map, c_neg_map,
                                                    True, False)
    sub = rows[1:]                                              # contiguous: the K sub-step poses of the count pass
    return _event_stream_run(what, 'boxroom', src, state, H, W, stamps, count_src=(src[0], _ptr(sub)) + src[2:])


# ------------------------------------------------------------------------------------------------
# The noisy event sensor (csrc/event_noise.hip; event_sim.EventSimulator(noise=...) drives it)
# ------------------------------------------------------------------------------------------------
def event_noise_params(what, noise, substeps, stamps):
    """The enslam_event_noise of one interval (host arithmetic only).  noise: dict with refractory (s), leak_rate (Hz),
    shot_rate (Hz), seed, interval; g = leak_rate * delta and q = shot_rate * delta with delta = (t_b - t_a) / K."""
    rho, lam, r = (float(noise.get(k, 0.0)) for k in ('refractory', 'leak_rate', 'shot_rate'))
    for name, v in (('refractory', rho), ('leak_rate', lam), ('shot_rate', r)):
        if not (v >= 0.0 and v < float('inf')):
            raise L.EnslamError(f"{what}: {name} must be finite and not negative (got {v})")
    delta = (stamps[1] - stamps[0]) / substeps
    q = r * delta
    if q > 1.0:
        raise L.EnslamError(f"{what}: shot_rate * sub-step length is {q} > 1: raise the number of sub-steps")
    seed, interval = int(noise.get('seed', 0)), int(noise.get('interval', 0))
    if not (0 <= seed < 2 ** 64 and 0 <= interval < 2 ** 32):
        raise L.EnslamError(f"{what}: seed must fit uint64 and interval uint32 (got {seed}, {interval})")
    n = L.EventNoiseParams()
    n.refractory, n.leak, n.shot, n.seed, n.interval, n.reserved = rho, lam * delta, q, seed, interval, 0
    return n


def event_noisy_images(prev, cur, state, t_last, stamps, noise, substeps=8, eps=1e-3, c_pos=0.2, c_neg=0.2, lut=None, levels=None,
                       c_pos_map=None, c_neg_map=None, stream=True):
    """One interval of the image route through the noisy sensor (enslam_event_noisy_images_*, enslam_hip.h): the arguments of
    `event_stream_images` plus `t_last` (float64 [H,W], updated in place like `state`) and `noise` (dict: refractory,
    leak_rate, shot_rate, seed, interval).  stream=True: (events, (t, x, y, p)) of the EMITTED events, two launches;
    stream=False: events alone, one launch."""
    what = "event_noisy_images"
    H, W, stamps, src = _event_image_source(what, prev, cur, state, stamps, substeps, eps, c_pos, c_neg, c_pos_map, c_neg_map, lut,
                                            levels, False)
    params = event_noise_params(what, noise, int(substeps), stamps)
    return _event_stream_run(what, 'images', src, state, H, W, stamps, noise=params, t_last=t_last, stream=stream)


def event_noisy_boxroom(room, poses, cam, state, t_last, stamps, noise, eps=1e-3, c_pos=0.2, c_neg=0.2, c_pos_map=None,
                        c_neg_map=None, stream=True):
    """One interval of the analytic route through the noisy sensor (enslam_event_noisy_boxroom_*, enslam_hip.h): the arguments
    of `event_stream_boxroom` (poses float64 [K+1,3|4,4], the previous frame's first) plus `t_last` and `noise` as in
    `event_noisy_images`; both passes read all K + 1 poses."""
    what = "event_noisy_boxroom"
    H, W, K, stamps, rows, src = _event_room_source(what, room, poses, cam, state, stamps, eps, c_pos, c_neg, c_pos_map, c_neg_map,
                                                    True, False)
    params = event_noise_params(what, noise, K, stamps)
    return _event_stream_run(what, 'boxroom', src, state, H, W, stamps, noise=params, t_last=t_last, stream=stream)


def event_accumulate(t, x, y, p, edges, H, W, want_unsaturated=False):
    """Bin a stream into count images (enslam_event_accumulate, enslam_hip.h).  t float64 [N], x, y uint16 [N], p uint8 [N] on
    one HIP device, in any order; edges: B + 1 ascending float64 times (a host sequence or array).  Event t goes to bin b
    where edges[b] < t <= edges[b+1].  Returns (counts uint8 [B,H,W,2] = (-, +) saturated at 255, dropped) -- dropped a pair
    of Python ints (outside every bin, outside the sensor) -- and with want_unsaturated also the uint32 counts as a third
    item.  The bins are processed in chunks of at most EVENT_ACCUMULATE_MAX_CELLS / (H W) so that the uint32 workspace stays
    bounded; the result does not depend on the chunking."""
    what = "event_accumulate"
    for name, a, dtype in (('t', t, torch.float64), ('x', x, torch.uint16), ('y', y, torch.uint16), ('p', p, torch.uint8)):
        if not torch.is_tensor(a):
            raise L.EnslamError(f"{what}: {name} must be a tensor (got {type(a).__name__})")
        _require_hip(a, f"{what}: {name}")
        if a.dtype != dtype or a.dim() != 1 or a.shape != t.shape or not a.is_contiguous() or a.device != t.device:
            raise L.EnslamError(f"{what}: {name} must be a contiguous {dtype} tensor [N] on the device of t (got {a.dtype} "
                                f"{tuple(a.shape)} on {a.device})")
    import numpy as np
    e = np.ascontiguousarray(np.asarray(edges.cpu() if torch.is_tensor(edges) else edges, dtype=np.float64))
    H, W = int(H), int(W)
    if e.ndim != 1 or e.size < 2:
        raise L.EnslamError(f"{what}: edges must be B + 1 >= 2 ascending times (got shape {e.shape})")
    if H <= 0 or W <= 0:
        raise L.EnslamError(f"{what}: the sensor must have pixels (got {H} x {W})")
    if not bool(np.all(e[:-1] <= e[1:])):
        raise L.EnslamError(f"{what}: edges must be ascending and hold no NaN")
    B, N, dev = int(e.size) - 1, int(t.shape[0]), t.device
    if H * W > EVENT_ACCUMULATE_MAX_CELLS:
        raise L.EnslamError(f"{what}: a sensor of {H} x {W} pixels is above the {EVENT_ACCUMULATE_MAX_CELLS} cells of one call")
    per = max(EVENT_ACCUMULATE_MAX_CELLS // (H * W), 1)
    lib = L.lib()
    with torch.cuda.device(dev):
        counts = torch.empty((B, H, W, 2), dtype=torch.uint8, device=dev)
        full = torch.empty((B, H, W, 2), dtype=torch.uint32, device=dev) if want_unsaturated else None
        edges_dev = torch.from_numpy(e).to(dev)
        dropped = torch.empty((-(-B // per), 2), dtype=torch.int64, device=dev)
        acc = None
        for c, b0 in enumerate(range(0, B, per)):
            b1 = min(b0 + per, B)
            if want_unsaturated:
                acc = full[b0:b1]
            elif acc is None or acc.shape[0] != b1 - b0:        # the workspace of one chunk, reused by the next
                acc = torch.empty((b1 - b0, H, W, 2), dtype=torch.uint32, device=dev)
            host = e[b0:b1 + 1]
            L.check(lib.enslam_event_accumulate(_ptr(t), _ptr(x), _ptr(y), _ptr(p), N,
                                                host.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                edges_dev.data_ptr() + 8 * b0, b1 - b0, H, W, _ptr(acc), _ptr(counts[b0:b1]),
                                                _ptr(dropped[c]), _stream()), "enslam_event_accumulate")
        d = dropped.cpu().tolist()
    chunks = len(d)
    sensor = d[0][1]
    # an event inside the range misses all chunks but its own, one outside misses every chunk
    by_time = sum(row[0] for row in d) - (N - sensor) * (chunks - 1)
    return (counts, (by_time, sensor), full) if want_unsaturated else (counts, (by_time, sensor))


# ------------------------------------------------------------------------------------------------
# Event-stream denoising (csrc/event_filter.hip; event_filter.EventFilter and event_filter.hot_pixels drive it)
# ------------------------------------------------------------------------------------------------
EVENT_CLASSES = ('kept', 'sensor', 'time', 'hot', 'refractory', 'unsupported')      # ENSLAM_EVENT_*: the value is the index
EVENT_NOT_TIME_ORDERED, EVENT_NOT_PIXEL_MAJOR = 1, 2
EVENT_FILTER_MAX_PIXELS = 1 << 28


def _event_arrays(what, t, x, y, p):
    for name, a, dtype in (('t', t, torch.float64), ('x', x, torch.uint16), ('y', y, torch.uint16), ('p', p, torch.uint8)):
        if not torch.is_tensor(a):
            raise L.EnslamError(f"{what}: {name} must be a tensor (got {type(a).__name__})")
        _require_hip(a, f"{what}: {name}")
        if a.dtype != dtype or a.dim() != 1 or a.shape != t.shape or not a.is_contiguous() or a.device != t.device:
            raise L.EnslamError(f"{what}: {name} must be a contiguous {dtype} tensor [N] on the device of t (got {a.dtype} "
                                f"{tuple(a.shape)} on {a.device})")
    if int(t.shape[0]) > 2147483647:
        raise L.EnslamError(f"{what}: at most 2^31 - 1 events per call (got {int(t.shape[0])})")


def _event_sensor(what, H, W):
    H, W = int(H), int(W)
    if H <= 0 or W <= 0 or H > 65536 or W > 65536 or H * W > EVENT_FILTER_MAX_PIXELS:
        raise L.EnslamError(f"{what}: the sensor must have 1..65536 rows and columns and at most 2^28 pixels (got {H} x {W})")
    return H, W


def _event_plane(what, name, a, dtype, H, W, dev):
    if not torch.is_tensor(a) or a.dtype != dtype or tuple(a.shape) != (H, W) or a.device != dev or not a.is_contiguous():
        raise L.EnslamError(f"{what}: {name} must be a contiguous {dtype} tensor [{H},{W}] on {dev} (got "
                            f"{(a.dtype, tuple(a.shape), a.device) if torch.is_tensor(a) else type(a).__name__})")


def event_pixel_counts(t, x, y, p, H, W, hot_mask=None):
    """Stage 0 of the event filter (enslam_event_pixel_counts, enslam_hip.h) on one HIP device: (cls uint8 [N], pix int32 [N],
    counts int32 [H,W], flags int).  cls holds the classes SENSOR / TIME / HOT or 0, pix the flat pixel index (-1 outside the
    sensor), counts the events per pixel that are neither SENSOR nor TIME, flags the bits EVENT_NOT_TIME_ORDERED and
    EVENT_NOT_PIXEL_MAJOR (one read-back).  hot_mask: uint8 [H,W] on the device or None."""
    what = "event_pixel_counts"
    _event_arrays(what, t, x, y, p)
    H, W = _event_sensor(what, H, W)
    dev, N = t.device, int(t.shape[0])
    if hot_mask is not None:
        _event_plane(what, 'hot_mask', hot_mask, torch.uint8, H, W, dev)
    with torch.cuda.device(dev):
        cls = torch.empty(N, dtype=torch.uint8, device=dev)
        pix = torch.empty(N, dtype=torch.int32, device=dev)
        counts = torch.empty((H, W), dtype=torch.int32, device=dev)
        flags = torch.empty(1, dtype=torch.int32, device=dev)
        L.check(L.lib().enslam_event_pixel_counts(_ptr(t), _ptr(x), _ptr(y), N, H, W, _ptr(hot_mask), _ptr(cls), _ptr(pix),
                                                  _ptr(counts), _ptr(flags), _stream()), "enslam_event_pixel_counts")
        return cls, pix, counts, int(flags.item())


def event_filter_order(t, cls, pix, counts, flags, hot_mask=None):
    """The ordering plumbing of the event filter, torch only: (order int32 [n_live], starts int64 [H W + 1], path).  order lists
    the live events (cls == 0) by (pixel, t, stream position); no sort where the stream is pixel-major already
    (path 'pixel_major'), one stable sort on the pixel where it is time-ordered ('time_ordered'), else a stable sort on t and
    one on the pixel ('unordered').  starts: the exclusive prefix sum of the live events per pixel."""
    idx = torch.nonzero(cls == 0).squeeze(1)
    if not flags & EVENT_NOT_PIXEL_MAJOR:
        order, path = idx, 'pixel_major'
    elif not flags & EVENT_NOT_TIME_ORDERED:
        order, path = idx[torch.sort(pix[idx], stable=True).indices], 'time_ordered'
    else:
        by_t = idx[torch.sort(t[idx], stable=True).indices]
        order, path = by_t[torch.sort(pix[by_t], stable=True).indices], 'unordered'
    live = counts if hot_mask is None else counts.masked_fill(hot_mask != 0, 0)
    starts = torch.zeros(live.numel() + 1, dtype=torch.int64, device=counts.device)
    torch.cumsum(live.reshape(-1), 0, dtype=torch.int64, out=starts[1:])
    return order.to(torch.int32), starts, path


def event_filter_stages(t, x, y, p, H, W, cls, pix, order, starts, t_last, t_seen, refractory=0.0, support_dt=None, mark=None):
    """Stages 1 and 2 and the compaction (enslam_event_filter_walk / _support / _compact) after event_pixel_counts and
    event_filter_order.  cls is completed in place (REFRACTORY, UNSUPPORTED), t_last and t_seen (float64 [H,W]) are updated in
    place.  Returns ((t, x, y, p) of the kept events in stream order, n_out).  mark: called with 'walk', 'support' and
    'compact' after the calls of each stage were enqueued (tools/bench_event_filter.py records device events there)."""
    what = "event_filter_stages"
    _event_arrays(what, t, x, y, p)
    H, W = _event_sensor(what, H, W)
    dev, N = t.device, int(t.shape[0])
    rho, dt = float(refractory), (0.0 if support_dt is None else float(support_dt))
    if not (0.0 <= rho < float('inf')) or not (0.0 <= dt < float('inf')):
        raise L.EnslamError(f"{what}: refractory and support_dt must be finite and not negative (got {refractory}, {support_dt})")
    _event_plane(what, 't_last', t_last, torch.float64, H, W, dev)
    _event_plane(what, 't_seen', t_seen, torch.float64, H, W, dev)
    for name, a, dtype, n in (('cls', cls, torch.uint8, N), ('pix', pix, torch.int32, N), ('order', order, torch.int32, None),
                              ('starts', starts, torch.int64, H * W + 1)):
        if not torch.is_tensor(a) or a.dtype != dtype or a.dim() != 1 or a.device != dev or not a.is_contiguous() or \
                (n is not None and int(a.shape[0]) != n):
            raise L.EnslamError(f"{what}: {name} must be a contiguous {dtype} tensor" + (f" [{n}]" if n is not None else "") + f" on {dev}")
    n_live = int(order.shape[0])
    if n_live > N:
        raise L.EnslamError(f"{what}: order lists {n_live} events of {N}")
    lib = L.lib()
    with torch.cuda.device(dev):
        s_times = torch.empty(n_live, dtype=torch.float64, device=dev)
        s_event = torch.empty(n_live, dtype=torch.int32, device=dev)
        s_count = torch.empty(H * W, dtype=torch.int32, device=dev)
        L.check(lib.enslam_event_filter_walk(_ptr(t), N, H, W, rho, _ptr(pix), _ptr(order), n_live, _ptr(starts), _ptr(cls),
                                             _ptr(t_last), _ptr(s_times), _ptr(s_event), _ptr(s_count), _stream()),
                "enslam_event_filter_walk")
        if mark is not None:
            mark('walk')
        L.check(lib.enslam_event_filter_support(N, H, W, 0 if support_dt is None else 1, dt, _ptr(pix), n_live, _ptr(starts),
                                                _ptr(cls), _ptr(t_last), _ptr(t_seen), _ptr(s_times), _ptr(s_event),
                                                _ptr(s_count), _stream()), "enslam_event_filter_support")
        if mark is not None:
            mark('support')
        ends = torch.cumsum(cls == 0, 0, dtype=torch.int64)
        n_out = int(ends[-1].item()) if N else 0
        out = (torch.empty(n_out, dtype=torch.float64, device=dev), torch.empty(n_out, dtype=torch.uint16, device=dev),
               torch.empty(n_out, dtype=torch.uint16, device=dev), torch.empty(n_out, dtype=torch.uint8, device=dev))
        L.check(lib.enslam_event_filter_compact(_ptr(t), _ptr(x), _ptr(y), _ptr(p), N, _ptr(cls), _ptr(ends), n_out,
                                                *(_ptr(a) for a in out), _stream()), "enslam_event_filter_compact")
        if mark is not None:
            mark('compact')
    return out, n_out


def event_class_counters(cls):
    """The counters of one filter call from its class array (uint8 [N], any device): dict n_in, sensor, time, hot, refractory,
    unsupported, n_out."""
    n = torch.bincount(cls.to(torch.int64), minlength=len(EVENT_CLASSES)).tolist() if cls.numel() else [0] * len(EVENT_CLASSES)
    out = dict(n_in=int(cls.numel()))
    out.update({name: int(n[k]) for k, name in enumerate(EVENT_CLASSES) if k})
    out['n_out'] = int(n[0])
    return out


# ------------------------------------------------------------------------------------------------
# Frame report (csrc/frame_report.hip; frame_vis.Visualizer and frame_vis.render_metrics drive it)
# ------------------------------------------------------------------------------------------------
SSIM_TILE = (16, 32)                    # ENSLAM_SSIM_TILE_H, ENSLAM_SSIM_TILE_W: output pixels of one workgroup
VIS_STAT_NAMES = ('n_valid', 'depth_abs_sum', 'color_sq_sum', 'color_sq_sum_valid')


def _report_image(what, name, t, shape, dev):
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or (dev is not None and t.device != dev):
        raise L.EnslamError(f"{what}: {name} must be a float tensor {list(shape)}" + (f" on {dev}" if dev is not None else "") +
                            f" (got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__})")
    if t.dtype not in (torch.float32, torch.float64):
        raise L.EnslamError(f"{what}: {name} must be float32 or float64 (got {t.dtype})")
    return t.detach().to(torch.float32).contiguous()


def vis_panels(gt_depth, gt_color, depth, color, gt_event=None, pred_event=None, gutter=8, title=16):
    """(sheet, stats): the figure of the reference's Visualizer as one uint8 image [R H + (R + 1) g + R t, 3 W + 4 g, 3] on the
    HIP device of the inputs -- rows depth, colour and, with gt_event / pred_event (float [h,w,2], both or neither), events;
    columns input, generated, residual; g = gutter, t = title, the white strip above each panel -- and stats, a float64 [8]
    device tensor {n_valid, sum |depth residual| over gt_depth > 0, sum of squared clipped colour error over everything and
    over gt_depth > 0} followed by the sums of the absolute terms (VIS_STAT_NAMES; enslam_vis_panels in enslam_hip.h holds
    every pixel rule).  gt_depth, depth: [H,W]; gt_color, color: [H,W,3]; float64 inputs are cast to float32 once.  Nothing is
    brought to the host here."""
    what = "vis_panels"
    if not isinstance(gt_depth, torch.Tensor) or not gt_depth.is_cuda:
        raise NotImplementedError("vis_panels needs a HIP device")
    if gt_depth.dim() != 2:
        raise L.EnslamError(f"{what}: gt_depth must be [H,W] (got {tuple(gt_depth.shape)})")
    H, W, dev = int(gt_depth.shape[0]), int(gt_depth.shape[1]), gt_depth.device
    gd = _report_image(what, 'gt_depth', gt_depth, (H, W), dev)
    gc = _report_image(what, 'gt_color', gt_color, (H, W, 3), dev)
    d = _report_image(what, 'depth', depth, (H, W), dev)
    c = _report_image(what, 'color', color, (H, W, 3), dev)
    if (gt_event is None) != (pred_event is None):
        raise L.EnslamError(f"{what}: gt_event and pred_event come together")
    ge = pe = None
    h = w = 0
    if gt_event is not None:
        if gt_event.dim() != 3 or gt_event.shape[2] != 2:
            raise L.EnslamError(f"{what}: gt_event must be [h,w,2] (got {tuple(gt_event.shape)})")
        h, w = int(gt_event.shape[0]), int(gt_event.shape[1])
        ge = _report_image(what, 'gt_event', gt_event, (h, w, 2), dev)
        pe = _report_image(what, 'pred_event', pred_event, (h, w, 2), dev)
    rows, g, t = 3 if ge is not None else 2, int(gutter), int(title)
    if g < 0 or t < 0:
        raise L.EnslamError(f"{what}: gutter and title must not be negative (got {gutter}, {title})")
    lib = L.lib()
    with torch.cuda.device(dev):
        nbytes = ctypes.c_int64()
        L.check(lib.enslam_vis_panels_workspace(H, W, rows, g, t, ctypes.byref(nbytes)), "enslam_vis_panels_workspace")
        ws = torch.empty(nbytes.value // 8, dtype=torch.float64, device=dev)
        sheet = torch.empty((rows * H + (rows + 1) * g + rows * t, 3 * W + 4 * g, 3), dtype=torch.uint8, device=dev)
        stats = torch.empty(8, dtype=torch.float64, device=dev)
        L.check(lib.enslam_vis_panels(_ptr(gd), _ptr(gc), _ptr(d), _ptr(c), _ptr(ge), _ptr(pe), H, W, h, w, g, t, _ptr(ws),
                                      nbytes.value, _ptr(sheet), _ptr(stats), _stream()), "enslam_vis_panels")
    return sheet, stats


def ssim(x, y, want_map=False):
    """Mean structural similarity of two images on a HIP device as a float64 [1] device tensor (with want_map the tuple (mean,
    map float64 [H-10,W-10,C])): x, y float [H,W,C] or [H,W], C 1 or 3, data range 1; 11 x 11 Gaussian window of sigma 1.5,
    K1 = 0.01, K2 = 0.03, population covariance, the mean over the interior and the channels, moments in float64
    (enslam_ssim, enslam_hip.h).  What skimage.metrics.structural_similarity(gaussian_weights=True, sigma=1.5,
    use_sample_covariance=False, data_range=1) and pytorch_msssim compute.  H, W >= 11."""
    what = "ssim"
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise NotImplementedError("ssim needs a HIP device")
    if x.dim() == 2:
        x = x[..., None]
        y = y[..., None] if isinstance(y, torch.Tensor) and y.dim() == 2 else y
    if x.dim() != 3:
        raise L.EnslamError(f"{what}: x must be [H,W,C] or [H,W] (got {tuple(x.shape)})")
    H, W, C, dev = int(x.shape[0]), int(x.shape[1]), int(x.shape[2]), x.device
    if C not in (1, 3):
        raise L.EnslamError(f"{what}: 1 or 3 channels (got {C})")
    if H < 11 or W < 11:
        raise L.EnslamError(f"{what}: the window is 11 x 11, the images are {H} x {W}")
    a = _report_image(what, 'x', x, (H, W, C), dev)
    b = _report_image(what, 'y', y, (H, W, C), dev)
    lib = L.lib()
    with torch.cuda.device(dev):
        nbytes = ctypes.c_int64()
        L.check(lib.enslam_ssim_workspace(H, W, C, ctypes.byref(nbytes)), "enslam_ssim_workspace")
        ws = torch.empty(nbytes.value // 8, dtype=torch.float64, device=dev)
        mean = torch.empty(1, dtype=torch.float64, device=dev)
        smap = torch.empty((H - 10, W - 10, C), dtype=torch.float64, device=dev) if want_map else None
        L.check(lib.enslam_ssim(_ptr(a), _ptr(b), H, W, C, _ptr(ws), nbytes.value, _ptr(mean), _ptr(smap), _stream()),
                "enslam_ssim")
    return (mean, smap) if want_map else mean


# ------------------------------------------------------------------------------------------------
# event-generation-model loss (csrc/event_model.hip; event_model.py is the caller)
# ------------------------------------------------------------------------------------------------
EVENT_MODEL_TILE, EVENT_MODEL_MAX_KERNELS, EVENT_MODEL_MAX_KSIZE = 16, 4, 31
_event_model_host = {}


def event_model_kernels(kernel_sizes, kernel_weights):
    """The host arrays of enslam_event_model_loss for these Gaussian kernels: (K, ksizes int32 [K], weights float32 [K], taps
    float32 [K][EVENT_MODEL_MAX_KSIZE]) with the taps of event.gaussian_kernel1d (float32, the numbers event.gaussian_blur
    convolves with).  Raises EnslamError for what the entry refuses.  Cached per (sizes, weights)."""
    key = (tuple(int(k) for k in kernel_sizes), tuple(float(x) for x in kernel_weights))
    got = _event_model_host.get(key)
    if got is not None:
        return got
    from .event import gaussian_kernel1d
    ks, ws = key
    if len(ks) != len(ws):
        raise L.EnslamError(f"event_model_loss: {len(ks)} kernel sizes but {len(ws)} kernel weights")
    if len(ks) > EVENT_MODEL_MAX_KERNELS:
        raise L.EnslamError(f"event_model_loss: at most {EVENT_MODEL_MAX_KERNELS} Gaussian kernels (got {len(ks)})")
    for k in ks:
        if k <= 0 or k % 2 == 0:
            raise L.EnslamError(f"event_model_loss: kernel sizes must be odd and positive (got {k})")
        if k > EVENT_MODEL_MAX_KSIZE:
            raise L.EnslamError(f"event_model_loss: kernel sizes up to {EVENT_MODEL_MAX_KSIZE} (got {k})")
    K = len(ks)
    taps = (ctypes.c_float * (max(K, 1) * EVENT_MODEL_MAX_KSIZE))()
    for i, k in enumerate(ks):
        for t, v in enumerate(gaussian_kernel1d(k, dtype=torch.float32).tolist()):
            taps[i * EVENT_MODEL_MAX_KSIZE + t] = v
    got = _event_model_host[key] = (K, (ctypes.c_int32 * max(K, 1))(*ks), (ctypes.c_float * max(K, 1))(*ws), taps)
    return got


def event_model_loss(cur, prev, gt, c_neg=0.2, c_pos=0.2, eps=1e-3, kernel_sizes=(9,), kernel_weights=(1.0,), want_blurred=False):
    """enslam_event_model_loss (enslam_hip.h) on contiguous float32 HIP tensors cur, prev [h,w,3] and gt [h,w,2]: (pred
    float32 [h,w,2], sums float64 [K + 2] = the raw term, the K blurred terms, the loss, grad float32 [h,w,3] = dloss/dcur,
    blur_gt, blur_pred float32 [K,h,w,2] or None).  Two launches on the current stream, no synchronisation."""
    what = "event_model_loss"
    for name, t, ch in (('cur', cur, 3), ('prev', prev, 3), ('gt', gt, 2)):
        if not torch.is_tensor(t) or t.dim() != 3 or t.shape[2] != ch or t.dtype is not torch.float32 or not t.is_contiguous():
            raise L.EnslamError(f"{what}: {name} must be a contiguous float32 tensor [h,w,{ch}] (got "
                                f"{(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__})")
        _require_hip(t, name)
    h, w = int(cur.shape[0]), int(cur.shape[1])
    if tuple(prev.shape[:2]) != (h, w) or tuple(gt.shape[:2]) != (h, w) or prev.device != cur.device or gt.device != cur.device:
        raise L.EnslamError(f"{what}: cur, prev and gt must share one resolution and device (got {tuple(cur.shape)}, "
                            f"{tuple(prev.shape)}, {tuple(gt.shape)})")
    if not (c_neg > 0 and c_pos > 0 and eps > 0):
        raise L.EnslamError(f"{what}: c_neg, c_pos and eps must be positive (got {c_neg}, {c_pos}, {eps})")
    K, ksizes, weights, taps = event_model_kernels(kernel_sizes, kernel_weights)
    for i in range(K):
        if ksizes[i] // 2 >= min(h, w):
            raise L.EnslamError(f"{what}: kernel size {ksizes[i]} needs reflect padding of {ksizes[i] // 2} >= min(h, w) = "
                                f"{min(h, w)}, which is undefined")
    dev = cur.device
    nbytes = ctypes.c_int64(0)
    L.check(L.lib().enslam_event_model_workspace(h, w, K, ctypes.byref(nbytes)), "enslam_event_model_workspace")
    with torch.cuda.device(dev):
        ws = torch.empty(max(nbytes.value // 8, 1), dtype=torch.float64, device=dev)
        pred = torch.empty((h, w, 2), dtype=torch.float32, device=dev)
        grad = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        sums = torch.empty(K + 2, dtype=torch.float64, device=dev)
        bg = bp = None
        if want_blurred and K > 0:
            bg = torch.empty((K, h, w, 2), dtype=torch.float32, device=dev)
            bp = torch.empty((K, h, w, 2), dtype=torch.float32, device=dev)
        L.check(L.lib().enslam_event_model_loss(_ptr(cur), _ptr(prev), _ptr(gt), h, w, ctypes.c_float(c_neg), ctypes.c_float(c_pos),
                                                ctypes.c_float(eps), K, ksizes, weights, taps, _ptr(ws), ws.numel() * 8, _ptr(pred),
                                                _ptr(sums), _ptr(grad), _ptr(bg), _ptr(bp), _stream()), "enslam_event_model_loss")
    return pred, sums, grad, bg, bp


# ------------------------------------------------------------------------------------------------
# event motion compensation by contrast maximisation (csrc/event_cmax.hip; event_cmax.py is the caller)
# ------------------------------------------------------------------------------------------------
EVENT_CMAX_MODELS = {'flow': (0, 2), 'rotation': (1, 3)}            # name -> (ENSLAM_CMAX_*, P)
EVENT_CMAX_RIGID = 6                                                # 'rigid': its own entry point, P = 6, four drop counters
EVENT_CMAX_MAX_KSIZE = 31
EVENT_CMAX_REGS = {'divergence': 1, 'deformation': 2}               # name -> ENSLAM_CMAX_REG_*


def event_cmax_eval(t, x, y, p, H, W, calib, model, theta, t_ref, taps, signed=False, want_grad=True, want_blurred=False,
                    depth=None, reg=None):
    """enslam_event_cmax_eval (enslam_hip.h) on a stream on one HIP device: t float64 [N], x, y uint16 [N], p uint8 [N].  calib =
    (fx, fy, cx, cy) pinhole, model 'flow' or 'rotation', theta its P host numbers, taps the k float64 taps of the blur (a
    host sequence).  Returns (iwe int64 [H,W], blurred float64 [H,W] or None, stats float64 [2 + P] = (mu, f, df/dtheta...),
    dropped int64 [3] = (time, sensor, warp)) as device tensors; no synchronisation.
    model 'rigid' is enslam_event_cmax_rigid_eval: theta = (w, v), P = 6, depth a contiguous float32 [H,W] tensor on the
    stream's device (required; refused for the other models), dropped int64 [4] = (time, sensor, warp, depth).
    reg 'divergence' or 'deformation' is enslam_event_cmax_reg_eval for any of the three models: the same four tensors, bit for
    bit, and a fifth, reg_stats float64 [2 + P] = (R, M, dR/dtheta...), the collapse regulariser of the header."""
    what = "event_cmax_eval"
    if reg is not None and reg not in EVENT_CMAX_REGS:
        raise L.EnslamError(f"{what}: reg must be None or one of {sorted(EVENT_CMAX_REGS)} (got {reg!r})")
    _event_arrays(what, t, x, y, p)
    H, W = _event_sensor(what, H, W)
    rigid = model == 'rigid'
    if not rigid and model not in EVENT_CMAX_MODELS:
        raise L.EnslamError(f"{what}: model must be one of {sorted(EVENT_CMAX_MODELS) + ['rigid']} (got {model!r})")
    if rigid:
        _event_plane(what, 'depth', depth, torch.float32, H, W, t.device)
    elif depth is not None:
        raise L.EnslamError(f"{what}: model {model!r} takes no depth")
    code, P = (None, EVENT_CMAX_RIGID) if rigid else EVENT_CMAX_MODELS[model]
    import math
    th = [float(v) for v in theta]
    cal = [float(v) for v in calib]
    tp = [float(v) for v in taps]
    if len(th) != P or len(cal) != 4:
        raise L.EnslamError(f"{what}: model {model!r} takes {P} parameters and calib = (fx, fy, cx, cy) (got {len(th)}, {len(cal)})")
    if not all(math.isfinite(v) for v in th + cal + tp + [float(t_ref)]) or cal[0] == 0.0 or cal[1] == 0.0:
        raise L.EnslamError(f"{what}: theta, t_ref, the intrinsics and the taps must be finite, fx and fy not 0")
    k = len(tp)
    if k % 2 == 0 or k > EVENT_CMAX_MAX_KSIZE:
        raise L.EnslamError(f"{what}: the blur takes an odd number of taps up to {EVENT_CMAX_MAX_KSIZE} (got {k})")
    N, dev = int(t.shape[0]), t.device
    lib = L.lib()
    nbytes = ctypes.c_int64(0)
    if reg is not None:
        code = 2 if rigid else code
        L.check(lib.enslam_event_cmax_reg_workspace(H, W, N, code, ctypes.byref(nbytes)), "enslam_event_cmax_reg_workspace")
    elif rigid:
        L.check(lib.enslam_event_cmax_rigid_workspace(H, W, N, ctypes.byref(nbytes)), "enslam_event_cmax_rigid_workspace")
    else:
        L.check(lib.enslam_event_cmax_workspace(H, W, N, P, ctypes.byref(nbytes)), "enslam_event_cmax_workspace")
    with torch.cuda.device(dev):
        ws = torch.empty(max(nbytes.value // 8, 1), dtype=torch.float64, device=dev)
        iwe = torch.empty((H, W), dtype=torch.int64, device=dev)
        blurred = torch.empty((H, W), dtype=torch.float64, device=dev) if want_blurred else None
        stats = torch.empty(2 + P, dtype=torch.float64, device=dev)
        dropped = torch.empty(4 if rigid else 3, dtype=torch.int64, device=dev)
        if reg is not None:
            reg_stats = torch.empty(2 + P, dtype=torch.float64, device=dev)
            L.check(lib.enslam_event_cmax_reg_eval(_ptr(t), _ptr(x), _ptr(y), _ptr(p), N, H, W, cal[0], cal[1], cal[2], cal[3], code,
                                                   _ptr(depth) if rigid else None, (ctypes.c_double * P)(*th), float(t_ref),
                                                   1 if signed else 0, k, (ctypes.c_double * k)(*tp), _ptr(ws), ws.numel() * 8,
                                                   _ptr(iwe), _ptr(blurred), _ptr(stats), _ptr(dropped), EVENT_CMAX_REGS[reg],
                                                   _ptr(reg_stats), 1 if want_grad else 0, _stream()), "enslam_event_cmax_reg_eval")
            return iwe, blurred, stats, dropped, reg_stats
        if rigid:
            L.check(lib.enslam_event_cmax_rigid_eval(_ptr(t), _ptr(x), _ptr(y), _ptr(p), N, H, W, cal[0], cal[1], cal[2], cal[3],
                                                     _ptr(depth), (ctypes.c_double * P)(*th), float(t_ref), 1 if signed else 0, k,
                                                     (ctypes.c_double * k)(*tp), _ptr(ws), ws.numel() * 8, _ptr(iwe), _ptr(blurred),
                                                     _ptr(stats), _ptr(dropped), 1 if want_grad else 0, _stream()),
                    "enslam_event_cmax_rigid_eval")
            return iwe, blurred, stats, dropped
        L.check(lib.enslam_event_cmax_eval(_ptr(t), _ptr(x), _ptr(y), _ptr(p), N, H, W, cal[0], cal[1], cal[2], cal[3], code,
                                           (ctypes.c_double * P)(*th), float(t_ref), 1 if signed else 0, k,
                                           (ctypes.c_double * k)(*tp), _ptr(ws), ws.numel() * 8, _ptr(iwe), _ptr(blurred),
                                           _ptr(stats), _ptr(dropped), 1 if want_grad else 0, _stream()), "enslam_event_cmax_eval")
    return iwe, blurred, stats, dropped


# ------------------------------------------------------------------------------------------------
# depth forecast (csrc/depth_forecast.hip): a measured depth image warped into another pose and size (slam.py is the caller)
# ------------------------------------------------------------------------------------------------
def relative_camera_matrix(src_c2w, dst_c2w):
    """The 3 x 4 float64 numpy matrix M = (dst_c2w^-1 src_c2w)[:3] that takes source-camera coordinates to target-camera
    coordinates, computed on the host in float64 (c2w: [3,4] or [4,4], tensor or array, any device)."""
    import numpy as np

    def full(c):
        c = np.asarray(c.detach().cpu().double().numpy() if torch.is_tensor(c) else c, dtype=np.float64)
        m = np.eye(4)
        m[:3] = c[:3]
        return m
    return np.ascontiguousarray((np.linalg.inv(full(dst_c2w)) @ full(src_c2w))[:3])


def _depth_forecast_numpy(depth, cam, m, Ho, Wo, radius, z_near, fill):
    """The model of enslam_depth_forecast (enslam_hip.h) on a numpy float32 [H,W] image: the same float64 operations in the
    same order on whole arrays, the z-buffer by numpy.minimum.at on the bit patterns.  Returns float32 [Ho,Wo]."""
    import numpy as np
    H, W = depth.shape
    fx, fy, cx, cy = (np.float64(cam[k]) for k in ('fx', 'fy', 'cx', 'cy'))
    sx = np.float64(W - 1) / np.float64(Wo - 1) if Wo > 1 else np.float64(1.0)
    sy = np.float64(H - 1) / np.float64(Ho - 1) if Ho > 1 else np.float64(1.0)
    votes = np.full(Ho * Wo, 0xFFFFFFFF, dtype=np.uint32)
    with np.errstate(all='ignore'):
        d = depth.astype(np.float64)
        jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
        ok = (d > 0.0) & np.isfinite(d)
        d, jj, ii = d[ok], jj[ok], ii[ok]
        px, py = (ii - cx) / fx, -(jj - cy) / fy
        p0, p1, p2 = d * px, d * py, -d
        q = [((m[r, 0] * p0 + m[r, 1] * p1) + m[r, 2] * p2) + m[r, 3] for r in range(3)]
        z = -q[2]
        zf = z.astype(np.float32)
        ok = (z > z_near) & np.isfinite(zf)
        q0, q1, z, zf = q[0][ok], q[1][ok], z[ok], zf[ok]
        u, v = cx + fx * (q0 / z), cy - fy * (q1 / z)
        fi, fj = np.floor(u / sx + 0.5), np.floor(v / sy + 0.5)
        ok = (fi >= 0.0) & (fi <= Wo - 1) & (fj >= 0.0) & (fj <= Ho - 1)
        ok &= (np.abs(u - fi * sx) <= radius) & (np.abs(v - fj * sy) <= radius)
        np.minimum.at(votes, fj[ok].astype(np.int64) * Wo + fi[ok].astype(np.int64), zf[ok].view(np.uint32))
    votes = votes.reshape(Ho, Wo)
    none = votes == 0xFFFFFFFF
    out = np.where(none, np.uint32(0), votes)
    if fill:
        pad = np.zeros((Ho + 2, Wo + 2), dtype=np.uint32)
        pad[1:-1, 1:-1] = out                               # (no vote and outside the image: 0, below every voted value)
        best = np.zeros((Ho, Wo), dtype=np.uint32)
        for dj in range(3):
            for di in range(3):
                best = np.maximum(best, pad[dj:dj + Ho, di:di + Wo])
        out = np.where(none, best, out)
    return np.ascontiguousarray(out.astype(np.uint32)).view(np.float32)


def depth_forecast(depth, cam, M, out_size, radius=1.0, z_near=0.0, fill=True):
    """float32 [Ho,Wo]: the depth image `depth` (float32 [H,W], contiguous) of one camera warped into another camera and the
    strided (Ho, Wo) pixel centres of `tracker.image_rays_from_camera_tensor` -- enslam_depth_forecast (enslam_hip.h states the
    model in full).  cam: dict with fx, fy, cx, cy of the full-resolution image; M: the 3 x 4 (or 4 x 4) float64 matrix from
    source-camera to target-camera coordinates (`relative_camera_matrix`), on the host; radius: how far, in full-resolution
    pixels, a point may land from a target pixel's centre and still vote for it; z_near: points at or nearer are dropped;
    fill: an empty pixel takes the largest value among its 8 neighbours (one round).  0 where nothing is known.  A tensor on a
    HIP device runs csrc/depth_forecast.hip (no synchronisation), a CPU tensor the numpy route of the same model: the two
    return the same bits."""
    import math
    import numpy as np
    what = "depth_forecast"
    if not torch.is_tensor(depth) or depth.dtype is not torch.float32 or depth.dim() != 2:
        raise L.EnslamError(f"{what}: depth must be a float32 [H,W] tensor (got "
                            f"{getattr(depth, 'dtype', type(depth))} {tuple(getattr(depth, 'shape', ()))})")
    if not depth.is_contiguous():
        raise L.EnslamError(f"{what}: depth must be contiguous")
    H, W = int(depth.shape[0]), int(depth.shape[1])
    Ho, Wo = int(out_size[0]), int(out_size[1])
    if H < 1 or W < 1 or Ho < 1 or Wo < 1:
        raise L.EnslamError(f"{what}: image sizes must be at least 1 x 1 (got {H} x {W} -> {Ho} x {Wo})")
    if (Wo > 1 and W == 1) or (Ho > 1 and H == 1):
        raise L.EnslamError(f"{what}: an axis of one source pixel cannot be spread over several target pixels "
                            f"(got {H} x {W} -> {Ho} x {Wo})")
    if H * W > (1 << 30) or Ho * Wo > (1 << 30):
        raise L.EnslamError(f"{what}: at most 2^30 source and target pixels")
    m = np.asarray(M.detach().cpu().numpy() if torch.is_tensor(M) else M, dtype=np.float64)
    if m.shape not in ((3, 4), (4, 4)):
        raise L.EnslamError(f"{what}: M must be 3 x 4 or 4 x 4 (got shape {m.shape})")
    m = np.ascontiguousarray(m[:3])
    c = [float(cam[k]) for k in ('fx', 'fy', 'cx', 'cy')]
    radius, z_near = float(radius), float(z_near)
    if not all(math.isfinite(v) for v in c + [radius, z_near]) or not np.isfinite(m).all() or c[0] == 0.0 or c[1] == 0.0:
        raise L.EnslamError(f"{what}: the intrinsics, M, radius and z_near must be finite, fx and fy not 0")
    if radius < 0.0 or z_near < 0.0:
        raise L.EnslamError(f"{what}: radius and z_near must not be negative (got {radius}, {z_near})")
    if not depth.is_cuda:
        out = _depth_forecast_numpy(depth.detach().numpy(), dict(fx=c[0], fy=c[1], cx=c[2], cy=c[3]), m, Ho, Wo, radius, z_near,
                                    bool(fill))
        return torch.from_numpy(out.copy())
    dev = depth.device
    with torch.cuda.device(dev):
        out = torch.empty((Ho, Wo), dtype=torch.float32, device=dev)
        ws = torch.empty(Ho * Wo, dtype=torch.int32, device=dev)
        L.check(L.lib().enslam_depth_forecast(_ptr(depth), H, W, c[0], c[1], c[2], c[3], (ctypes.c_double * 12)(*m.reshape(-1)),
                                              Ho, Wo, radius, z_near, 1 if fill else 0, _ptr(ws), _ptr(out), _stream()),
                "enslam_depth_forecast")
    return out
