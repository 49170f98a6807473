"""Host-side mirror of the reference's call surface for the render path,

    scene   = rgbbox() | irreg()                       futhark/ray.fut:176, :223
    prepared = prepare_scene(h, w, scene)              futhark/ray.fut:241-244
    pixels  = render(h, w, prepared)                   futhark/ray.fut:246-247
    pixels  = render_image(objs, width, height, cam)   futhark/ray.fut:166-169

over the C ABI of libray_mi355x.so (include/rt_mi355x.h).  Pixels are the reference's packed
i32 `(r<<16)|(g<<8)|b`, row-major from the top row.  Every render launches HIP kernels on the
context's stream; there is no CPU path.
"""
import ctypes as C

import numpy as np

from ._lib import lib

VARIANT_AUTO, VARIANT_PIXEL, VARIANT_PERSISTENT, VARIANT_POOLED = 0, 1, 2, 3
MAX_DEPTH = 50          # ray.fut:154
PATH_ESCAPED, PATH_ABSORBED, PATH_TRUNCATED = 0, 1, 2   # rt_trace_paths's end codes (RT_PATH_*)
PAIRS_TARGETS, PAIRS_DIRECTIONS = 0, 1                  # rt_visible_pairs's modes (RT_PAIRS_*)
ROWS_PER_TILE = 8       # cyclic row-tile height of the multi-GPU partition


class RtError(RuntimeError):
    pass


class Context:
    """One HIP device + one stream.  stream=None: the context owns a private stream.
    Otherwise `stream` is a raw hipStream_t as an int, e.g.
    torch.cuda.current_stream().cuda_stream (0 = the default stream), so that launches order
    with torch work and torch.cuda.Event timing sees them."""

    def __init__(self, device=-1, stream=None, devices=None):
        """devices: a list of HIP device ordinals -> ONE context over several GPUs (rt_context_create_multi):
        whole frames are cut into cyclic row tiles over them and gathered on devices[0]."""
        h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int * len(devices))(*[int(d) for d in devices])
            rc = lib.rt_context_create_multi(C.byref(h), arr, len(devices))
        else:
            rc = lib.rt_context_create(C.byref(h), int(device), C.c_void_p(stream or 0), 0 if stream is None else 1)
        if rc != 0 or not h.value:
            raise RtError(f"rt_context_create failed (code {rc}): no usable HIP device; "
                          "raytracers_amd has no CPU fallback")
        self._h = h

    # -- plumbing
    def _check(self, rc):
        if rc != 0:
            raise RtError(lib.rt_last_error(self._h).decode() or f"error code {rc}")

    def close(self):
        if getattr(self, "_h", None):
            lib.rt_context_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._check(lib.rt_context_sync(self._h))

    @property
    def num_devices(self):
        return int(lib.rt_context_num_devices(self._h))

    @property
    def gather_mode(self):
        return lib.rt_context_gather_mode(self._h).decode()

    @property
    def last_launch(self):
        """what the last render entry enqueued: family, tickets (pixel list / ordered tiles / raster), instantiation, launch shape, and for a pooled render
        launch whether it stops chains whose light is exactly zero ("dark=0|1", option dark_stop: -1 default, 0 never, 1 also the instrumented launch)
        and whether it drops sphere tests whose own widened box the ray misses ("leaf_box=0|1", option leaf_box, the same three values);
        "entry=lists|root": whether new primary rays start at their tile's entry list (option entry_lists: -1 default, 0 never, 1 wherever legal)"""
        return lib.rt_context_last_launch(self._h).decode()

    def entry_counts(self):
        """option entry_count = 1: what the last pooled render launch counted -- {"lists": primary rays started from their tile's entry list, "fallbacks": rays
        that had a list and took the root (their wave's leaf list had no room), "waves": waves that counted (0: the launch carried no table), "per_wave": (waves, 2)}"""
        lists, falls, nw = C.c_uint64(), C.c_uint64(), C.c_int64()
        self._check(lib.rt_context_entry_counts(self._h, C.byref(lists), C.byref(falls), C.byref(nw), None, 0))
        per = np.zeros((nw.value, 2), np.uint64)
        if nw.value:
            self._check(lib.rt_context_entry_counts(self._h, None, None, None, per.ctypes.data_as(C.POINTER(C.c_uint64)), nw.value))
        return {"lists": lists.value, "fallbacks": falls.value, "waves": nw.value, "per_wave": per}

    def entry_info(self):
        """what last_launch has no room for: {"colour_lds": the last pooled render launch read the winner's colour from LDS, "flags_const": its kernel had
        the leaf filter and the dark stop compiled in (both False for a launch that says entry=root), "tables_built": tables of entry lists this context's
        launches have built, "tables_kept": launches that found their view's table in place (option entry_keep)}"""
        col, const, built, kept = C.c_int32(), C.c_int32(), C.c_uint64(), C.c_uint64()
        self._check(lib.rt_context_entry_info(self._h, C.byref(col), C.byref(const), C.byref(built), C.byref(kept)))
        return {"colour_lds": bool(col.value), "flags_const": bool(const.value), "tables_built": built.value, "tables_kept": kept.value}

    def exit_info(self):
        """exit lists (option exit_lists: -1 default, 0 never, 1 wherever legal): {"active": the last pooled render launch started its scattered rays at
        their origin sphere's exit list, "dmax": the depth the lists resume at (compile time), "tables_built" / "tables_kept": times this context's launches
        built the tables / found them in place, "lists" / "fallbacks": under option entry_count = 1 the scattered rays of that launch that started from a
        list / had one and took the root}"""
        act, dmax = C.c_int32(), C.c_int32()
        built, kept, lists, falls = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(lib.rt_context_exit_info(self._h, C.byref(act), C.byref(dmax), C.byref(built), C.byref(kept), C.byref(lists), C.byref(falls)))
        return {"active": bool(act.value), "dmax": dmax.value, "tables_built": built.value, "tables_kept": kept.value, "lists": lists.value,
                "fallbacks": falls.value}

    def wide_info(self):
        """the twenty-wave shape's constants (option wide_const: -1 default, 0 the generic four-wave kernels): {"shape_const": the last pooled launch ran a
        kernel with lds_nodes = lds_sph = 0 and two ray planes compiled in}; last_launch reads the same either way"""
        const = C.c_int32()
        self._check(lib.rt_context_wide_info(self._h, C.byref(const)))
        return {"shape_const": bool(const.value)}

    @property
    def rccl_ranks(self):
        """ranks of the RCCL communicator behind a multi-device context's gather (0: RCCL is not what carries it)"""
        return int(lib.rt_context_rccl_ranks(self._h))

    def set_variant(self, v):
        self._check(lib.rt_context_set_variant(self._h, int(v)))

    def set_option(self, name, value):
        self._check(lib.rt_context_set_option(self._h, name.encode(), int(value)))

    def device_info(self):
        dev, cus, lds = C.c_int(), C.c_int(), C.c_int()
        name = C.create_string_buffer(64)
        self._check(lib.rt_context_device_info(self._h, C.byref(dev), C.byref(cus), C.byref(lds), name, 64))
        return {"device": dev.value, "num_cu": cus.value, "lds_bytes": lds.value, "arch": name.value.decode()}

    # -- scenes
    def _scene(self, fn, *args):
        h = C.c_void_p()
        self._check(fn(self._h, C.byref(h), *args))
        return Scene(self, h)

    def rgbbox(self):
        return self._scene(lib.rt_scene_rgbbox)

    def irreg(self):
        return self._scene(lib.rt_scene_irreg)

    def floor(self, n, k):
        return self._scene(lib.rt_scene_floor, int(n), float(k))

    def scene(self, name):
        if name == "rgbbox":
            return self.rgbbox()
        if name == "irreg":
            return self.irreg()
        if name == "big":
            return self.floor(1000, 6000.0)
        raise ValueError(f"unknown scene {name!r}")

    def scene_from_spheres(self, spheres7, look_from, look_at, fov):
        s = np.ascontiguousarray(spheres7, dtype=np.float32)
        if s.ndim != 2 or s.shape[1] != 7:
            raise ValueError("spheres7 must be (n, 7): pos.xyz, colour.rgb, radius")
        lf = (C.c_float * 3)(*look_from)
        la = (C.c_float * 3)(*look_at)
        h = C.c_void_p()
        self._check(lib.rt_scene_from_spheres(self._h, C.byref(h), s.ctypes.data, s.shape[0], lf, la, float(fov)))
        return Scene(self, h)

    # -- device memory for callers without an allocator of their own
    def alloc_i32(self, count):
        return DeviceBuffer(self, int(count) * 4)


class DeviceBuffer:
    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        p = C.c_void_p()
        ctx._check(lib.rt_device_alloc(ctx._h, C.byref(p), nbytes))
        self.ptr = p.value

    def as_torch(self, shape):
        """zero-copy torch int32 view of the buffer (the buffer must outlive it)"""
        import torch
        n = int(np.prod(shape))
        assert n * 4 <= self.nbytes
        iface = {"shape": tuple(int(x) for x in shape), "typestr": "<i4", "data": (int(self.ptr), False), "version": 2}
        holder = type("_CudaArray", (), {"__cuda_array_interface__": iface})()
        # (the device that owns the buffer, not torch's current one: a context on another GPU would get a mislabelled tensor)
        return torch.as_tensor(holder, device=torch.device("cuda", self.ctx.device_info()["device"]))

    def to_host(self, shape, dtype=np.int32):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        self.ctx._check(lib.rt_copy_to_host(self.ctx._h, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr and self.ctx._h:
            lib.rt_device_free(self.ctx._h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Scene:
    def __init__(self, ctx, h):
        self.ctx, self._h = ctx, h

    @property
    def num_spheres(self):
        return int(lib.rt_scene_num_spheres(self._h))

    def free(self):
        if self._h and self.ctx._h:
            lib.rt_scene_free(self.ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Prepared:
    """prepared_scene = {objs: bvh, cam: camera} (ray.fut:239), resident on the device."""

    def __init__(self, ctx, h, height, width):
        self.ctx, self._h, self.h, self.w = ctx, h, int(height), int(width)

    @property
    def num_spheres(self):
        return int(lib.rt_prepared_num_spheres(self._h))

    @property
    def height(self):
        """levels of inner nodes on the longest root-to-leaf path of the BVH"""
        return int(lib.rt_prepared_height(self._h))

    def camera(self):
        cam = np.empty(12, dtype=np.float32)
        self.ctx._check(lib.rt_prepared_get_camera(self.ctx._h, self._h, cam.ctypes.data))
        return cam

    def bvh_arrays(self):
        """Canonical {L, I} of bvh.fut:28 copied back from the device (for parity checks)."""
        n = self.num_spheres
        ni = n - 1
        A = {"L": np.empty((n, 7), np.float32), "bmin": np.empty((ni, 3), np.float32),
             "bmax": np.empty((ni, 3), np.float32), "left": np.empty(ni, np.int32),
             "right": np.empty(ni, np.int32), "parent": np.empty(ni, np.int32)}
        self.ctx._check(lib.rt_prepared_get_bvh(self.ctx._h, self._h, *[A[k].ctypes.data for k in
                                                                       ("L", "bmin", "bmax", "left", "right", "parent")]))
        return A

    def sphere_ids(self):
        """(n,) int32 numpy array: ids[i] = the caller's index of L[i] (rt_prepared_get_sphere_ids) -- L, the order every query's sphere
        index refers to, is Morton order; ids maps it back to the order of the spheres the scene was prepared (or last updated) from."""
        n = self.num_spheres
        buf = DeviceBuffer(self.ctx, max(4 * n, 4))
        try:
            self.sphere_ids_into(buf.ptr)
            return buf.to_host((n,))
        finally:
            buf.free()

    def sphere_ids_into(self, ids_ptr):
        """Enqueue the copy of the n sphere ids (int32) to the device pointer ids_ptr.  Asynchronous: ctx.sync() completes it."""
        self.ctx._check(lib.rt_prepared_get_sphere_ids(self.ctx._h, self._h, C.c_void_p(ids_ptr)))

    def update_spheres(self, spheres):
        """Rebuild this prepared scene in place from new spheres (rt_prepared_update_spheres): the same count, camera and handle;
        every view's tile order / pixel list starts afresh.  `spheres` as for prepare_scene_from_spheres.  Returns after the build:
        the caller may then overwrite the source."""
        ptr, n, keep = _device_spheres(self.ctx, spheres)
        try:
            self.ctx._check(lib.rt_prepared_update_spheres(self.ctx._h, self._h, C.c_void_p(ptr), n))
        finally:
            if keep is not None:
                keep.free()

    def set_groups(self, groups):
        """Give every sphere a 32-bit group word (rt_prepared_set_groups), in the CALLER's sphere order -- the order sphere_ids() maps back
        to -- for the mask= keyword of intersect_rays, occluded_rays, nearest_spheres and spheres_within: a query with mask m sees sphere j
        iff groups[j] & m != 0.  `groups`: an (n,) integer numpy array with values in [0, 2^32), an (n,) contiguous int32 or uint32 torch
        tensor on the context's device (its bits are the words; copied on the context's stream), or None: the scene has no groups again.
        The words survive update_spheres: sphere c of the caller's order keeps word c."""
        if groups is None:
            self.ctx._check(lib.rt_prepared_set_groups(self.ctx._h, self._h, None, 0))
            return
        with _Scope(self.ctx) as s:
            ptr, n = _device_words(s, groups, "groups", None)
            self.ctx._check(lib.rt_prepared_set_groups(self.ctx._h, self._h, C.c_void_p(ptr), n))
            self.ctx.sync()   # (the copy has run: the scope's buffer may go)

    def groups(self):
        """(groups (n,) uint32 in L order, node_groups (n - 1,) uint32) numpy arrays (rt_prepared_get_groups): groups[i] is the word of L[i],
        node_groups[v] the OR of the words of every sphere below inner node v, numbered as in bvh_arrays()."""
        n = self.num_spheres
        g, ng = DeviceBuffer(self.ctx, 4 * n), DeviceBuffer(self.ctx, max(4 * (n - 1), 4))
        try:
            self.groups_into(g.ptr, ng.ptr)
            return g.to_host((n,), np.uint32), ng.to_host((n - 1,), np.uint32)
        finally:
            g.free()
            ng.free()

    def groups_into(self, groups_ptr=None, node_groups_ptr=None):
        """Enqueue the copies of groups() to device pointers (n and n - 1 uint32; either may be None, not both).  Asynchronous."""
        self.ctx._check(lib.rt_prepared_get_groups(self.ctx._h, self._h, C.c_void_p(groups_ptr), C.c_void_p(node_groups_ptr)))

    def stats(self, max_depth=MAX_DEPTH):
        s = (C.c_uint64 * 3)()
        self.ctx._check(lib.rt_render_stats(self.ctx._h, self._h, self.h, self.w, int(max_depth), s))
        return {"rays": int(s[0]), "box_tests": int(s[1]), "leaf_tests": int(s[2])}

    def free(self):
        if self._h and self.ctx._h:
            lib.rt_prepared_free(self.ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def prepare_scene(h, w, scene):
    """entry prepare_scene h w scene (ray.fut:241): BVH build + camera for an h x w image."""
    ctx = scene.ctx
    p = C.c_void_p()
    ctx._check(lib.rt_prepare_scene(ctx._h, C.byref(p), int(h), int(w), scene._h))
    return Prepared(ctx, p, h, w)


def _device_spheres(ctx, spheres):
    """(pointer, n, keep-alive) for `spheres` (n x 7 {pos.xyz, colour.rgb, radius}): a numpy array is uploaded to a fresh device
    buffer; a contiguous float32 torch tensor on the context's device is used in place."""
    if hasattr(spheres, "data_ptr"):
        dev = ctx.device_info()["device"]
        if str(spheres.dtype) != "torch.float32" or not spheres.is_contiguous() or spheres.device.type != "cuda" or spheres.device.index != dev:
            raise ValueError(f"spheres: a contiguous float32 tensor on cuda:{dev} is required")
        if spheres.dim() != 2 or spheres.shape[1] != 7:
            raise ValueError("spheres must be (n, 7): pos.xyz, colour.rgb, radius")
        return spheres.data_ptr(), int(spheres.shape[0]), None
    a = np.ascontiguousarray(spheres, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 7:
        raise ValueError("spheres must be (n, 7): pos.xyz, colour.rgb, radius")
    buf = DeviceBuffer(ctx, max(a.nbytes, 4))
    try:
        if a.nbytes:
            ctx._check(lib.rt_copy_to_device(ctx._h, C.c_void_p(buf.ptr), a.ctypes.data, a.nbytes))
    except BaseException:
        buf.free()
        raise
    return buf.ptr, a.shape[0], buf


def prepare_scene_from_spheres(ctx, spheres, h, w, look_from, look_at, fov):
    """prepare_scene of the scene {look_from, look_at, fov, spheres} straight from device memory (rt_prepare_scene_device): the same
    prepared scene as prepare_scene(h, w, ctx.scene_from_spheres(...)) on the same bytes.  `spheres`: (n, 7) float32 -- a numpy array
    (uploaded to a temporary device buffer) or a contiguous torch tensor on the context's device, read in place on the context's stream."""
    ptr, n, keep = _device_spheres(ctx, spheres)
    lf = (C.c_float * 3)(*look_from)
    la = (C.c_float * 3)(*look_at)
    p = C.c_void_p()
    try:
        ctx._check(lib.rt_prepare_scene_device(ctx._h, C.byref(p), int(h), int(w), C.c_void_p(ptr), n, lf, la, float(fov)))
    finally:
        if keep is not None:
            keep.free()
    return Prepared(ctx, p, h, w)


def part_rows(h, part=0, nparts=1, rows_per_tile=ROWS_PER_TILE):
    return int(lib.rt_part_rows(int(h), int(rows_per_tile), int(part), int(nparts)))


def render_into(out_ptr, h, w, prepared, max_depth=MAX_DEPTH, part=0, nparts=1, rows_per_tile=ROWS_PER_TILE, cam=None):
    """Enqueue a render of part `part` of `nparts` into the device pointer `out_ptr`
    (part_rows(h, part, nparts) * w int32).  Asynchronous: ctx.sync() completes it."""
    ctx = prepared.ctx
    if cam is None:
        ctx._check(lib.rt_render_part(ctx._h, prepared._h, int(h), int(w), int(max_depth), int(rows_per_tile),
                                      int(part), int(nparts), C.c_void_p(out_ptr)))
    else:
        c = np.ascontiguousarray(cam, dtype=np.float32)
        assert c.size == 12
        ctx._check(lib.rt_render_image(ctx._h, prepared._h, int(w), int(h), c.ctypes.data, int(max_depth),
                                       int(rows_per_tile), int(part), int(nparts), C.c_void_p(out_ptr)))


def render_batch_into(out_ptr, h, w, prepared, nframes, frame_stride=None, cams=None, max_depth=MAX_DEPTH, part=0, nparts=1,
                      rows_per_tile=ROWS_PER_TILE):
    """`nframes` frames in ONE launch (rt_render_batch): frame f -> out_ptr + 4 * f * frame_stride (default: packed,
    part_rows * w elements apart), traced through cams[f] (nframes x 12 floats) or, cams=None, the prepared camera."""
    ctx = prepared.ctx
    if frame_stride is None:
        frame_stride = part_rows(h, part, nparts, rows_per_tile) * w
    cp = None
    if cams is not None:
        c = np.ascontiguousarray(cams, dtype=np.float32)
        assert c.size == 12 * nframes
        cp = c.ctypes.data
    ctx._check(lib.rt_render_batch(ctx._h, prepared._h, int(h), int(w), int(max_depth), int(rows_per_tile), int(part), int(nparts),
                                   int(nframes), C.c_void_p(cp), int(frame_stride), C.c_void_p(out_ptr)))


def render_inplace_into(image_ptr, h, w, prepared, nframes=1, frame_stride=None, cams=None, max_depth=MAX_DEPTH, part=0, nparts=1,
                        rows_per_tile=ROWS_PER_TILE):
    """Part `part` of `nparts` of `nframes` frames stored IN PLACE (rt_render_part_inplace): image_ptr is the FULL image
    (frame f at image_ptr + 4 * f * frame_stride, default h * w) -- possibly another device's memory (a peer allocation or
    an ipc_import'ed buffer): the pixel stores then are the framebuffer exchange."""
    ctx = prepared.ctx
    cp = None
    if cams is not None:
        c = np.ascontiguousarray(cams, dtype=np.float32)
        assert c.size == 12 * nframes
        cp = c.ctypes.data
    ctx._check(lib.rt_render_part_inplace(ctx._h, prepared._h, int(h), int(w), int(max_depth), int(rows_per_tile), int(part), int(nparts),
                                          int(nframes), C.c_void_p(cp), int(h * w if frame_stride is None else frame_stride),
                                          C.c_void_p(image_ptr)))


def ipc_export(ctx, dev_ptr):
    """64 opaque bytes naming the device allocation at dev_ptr (a DeviceBuffer's pointer) for the other processes of the node"""
    h = (C.c_ubyte * 64)()
    ctx._check(lib.rt_ipc_export(ctx._h, C.c_void_p(dev_ptr), h))
    return bytes(h)


def ipc_import(ctx, handle64):
    """a device pointer to another process's exported allocation (valid until ipc_close)"""
    assert len(handle64) == 64
    h = (C.c_ubyte * 64).from_buffer_copy(handle64)
    p = C.c_void_p()
    ctx._check(lib.rt_ipc_import(ctx._h, h, C.byref(p)))
    return p.value


def ipc_close(ctx, dev_ptr):
    ctx._check(lib.rt_ipc_close(ctx._h, C.c_void_p(dev_ptr)))


def render(h, w, prepared, max_depth=MAX_DEPTH):
    """entry render h w prepared (ray.fut:246): returns the [h][w]i32 image as a numpy array."""
    buf = prepared.ctx.alloc_i32(h * w)
    try:
        render_into(buf.ptr, h, w, prepared, max_depth)
        return buf.to_host((h, w))
    finally:
        buf.free()


def render_image(objs, width, height, cam, max_depth=MAX_DEPTH):
    """render_image objs width height cam (ray.fut:166): explicit camera (12 floats)."""
    buf = objs.ctx.alloc_i32(height * width)
    try:
        render_into(buf.ptr, height, width, objs, max_depth, cam=cam)
        return buf.to_host((height, width))
    finally:
        buf.free()


def render_timed(out_ptr, h, w, prepared, warmup, iters, max_depth=MAX_DEPTH, part=0, nparts=1,
                 rows_per_tile=ROWS_PER_TILE):
    """`iters` back-to-back launches timed with HIP events on the context's stream; returns ms per launch."""
    ctx = prepared.ctx
    ms = np.zeros(iters, dtype=np.float32)
    ctx._check(lib.rt_render_timed(ctx._h, prepared._h, int(h), int(w), int(max_depth), int(rows_per_tile), int(part),
                                   int(nparts), C.c_void_p(out_ptr), int(warmup), int(iters), ms.ctypes.data))
    return ms


def place_part(ctx, h, w, part, nparts, part_ptr, image_ptr, rows_per_tile=ROWS_PER_TILE):
    ctx._check(lib.rt_place_part(ctx._h, int(h), int(w), int(rows_per_tile), int(part), int(nparts),
                                 C.c_void_p(part_ptr), C.c_void_p(image_ptr)))


def place_parts(ctx, h, w, nparts, pad_rows, stacked_ptr, image_ptr, rows_per_tile=ROWS_PER_TILE, part_stride=None):
    """All gathered parts -> the h x w image, one kernel.  Part p's packed rows start at
    stacked_ptr + 4 * p * part_stride (default: pad_rows * w, i.e. nparts x pad_rows x w)."""
    if part_stride is None:
        ctx._check(lib.rt_place_parts(ctx._h, int(h), int(w), int(rows_per_tile), int(nparts), int(pad_rows),
                                      C.c_void_p(stacked_ptr), C.c_void_p(image_ptr)))
    else:
        ctx._check(lib.rt_place_parts_strided(ctx._h, int(h), int(w), int(rows_per_tile), int(nparts), int(part_stride),
                                              C.c_void_p(stacked_ptr), C.c_void_p(image_ptr)))


def place_parts_batch(ctx, h, w, nparts, part_stride, nframes, frame_stride_in, stacked_ptr, images_ptr, frame_stride_out=None,
                      rows_per_tile=ROWS_PER_TILE):
    """All gathered parts of `nframes` frames -> nframes h x w images, ONE kernel (rt_place_parts_batch): inside part p
    (at stacked_ptr + 4 * p * part_stride) frame f's packed rows start f * frame_stride_in elements in; image f at
    images_ptr + 4 * f * frame_stride_out (default h * w)."""
    ctx._check(lib.rt_place_parts_batch(ctx._h, int(h), int(w), int(rows_per_tile), int(nparts), int(part_stride), int(nframes),
                                        int(frame_stride_in), int(h * w if frame_stride_out is None else frame_stride_out),
                                        C.c_void_p(stacked_ptr), C.c_void_p(images_ptr)))


# -- caller-supplied rays: objs_hit / ray_colour (ray.fut:76-86, :126-148) on a prepared scene.  Rays are n x 6 float32
# {origin.xyz, dir.xyz} in the context's device memory.

def trace_rays_into(rays_ptr, n, prepared, colour_ptr=None, pixel_ptr=None, max_depth=MAX_DEPTH):
    """Enqueue ray_colour of `n` rays at the device pointer `rays_ptr`: colours (n x 3 float32) to colour_ptr and / or packed
    pixels (n int32) to pixel_ptr (rt_trace_rays).  Asynchronous: ctx.sync() completes it."""
    ctx = prepared.ctx
    ctx._check(lib.rt_trace_rays(ctx._h, prepared._h, int(n), C.c_void_p(rays_ptr), int(max_depth), C.c_void_p(colour_ptr),
                                 C.c_void_p(pixel_ptr)))


def intersect_rays_into(rays_ptr, n, prepared, index_ptr, hit_ptr=None, t_min=0.0, t_max=1e9):
    """Enqueue objs_hit bvh r t_min t_max of `n` rays (rt_intersect_rays): sphere index (n int32, -1 for none) to index_ptr,
    {t, p.xyz, normal.xyz} (n x 7 float32) to hit_ptr if given."""
    ctx = prepared.ctx
    ctx._check(lib.rt_intersect_rays(ctx._h, prepared._h, int(n), C.c_void_p(rays_ptr), float(t_min), float(t_max),
                                     C.c_void_p(index_ptr), C.c_void_p(hit_ptr)))


def occluded_rays_into(rays_ptr, n, prepared, out_ptr, t_min=0.0, t_max=1e9):
    """Enqueue the occlusion of `n` rays over (t_min, t_max) (rt_occluded_rays): n bytes at out_ptr, 1 where some sphere the BVH
    walk reaches has a root strictly inside the interval, else 0."""
    ctx = prepared.ctx
    ctx._check(lib.rt_occluded_rays(ctx._h, prepared._h, int(n), C.c_void_p(rays_ptr), float(t_min), float(t_max),
                                    C.c_void_p(out_ptr)))


def intersect_rays_ranged_into(rays_ptr, n, prepared, t_min_ptr, t_max_ptr, index_ptr, hit_ptr=None):
    """intersect_rays_into with ray i's own interval (t_min_ptr[i], t_max_ptr[i]): n float32 each at device pointers
    (rt_intersect_rays_ranged).  A ray whose interval fails 0 <= t_min <= t_max <= 1e9 (NaN included) is a miss."""
    ctx = prepared.ctx
    ctx._check(lib.rt_intersect_rays_ranged(ctx._h, prepared._h, int(n), C.c_void_p(rays_ptr), C.c_void_p(t_min_ptr), C.c_void_p(t_max_ptr),
                                            C.c_void_p(index_ptr), C.c_void_p(hit_ptr)))


def occluded_rays_ranged_into(rays_ptr, n, prepared, t_min_ptr, t_max_ptr, out_ptr):
    """occluded_rays_into with ray i's own interval (t_min_ptr[i], t_max_ptr[i]) (rt_occluded_rays_ranged); an invalid interval
    gives 0."""
    ctx = prepared.ctx
    ctx._check(lib.rt_occluded_rays_ranged(ctx._h, prepared._h, int(n), C.c_void_p(rays_ptr), C.c_void_p(t_min_ptr), C.c_void_p(t_max_ptr),
                                           C.c_void_p(out_ptr)))


def multi_hit_rays_into(rays_ptr, n, prepared, k, count_ptr, index_ptr, root_ptr=None, hit_ptr=None, t_min=0.0, t_max=1e9):
    """Enqueue the first k (1 <= k <= 32) sphere crossings of `n` rays over (t_min, t_max), ordered by (t, sphere, root)
    (rt_multi_hit_rays): their count (n int32, not capped at k) to count_ptr, sphere indices (n x k int32, -1 past the count) to
    index_ptr, roots (n x k uint8: 1 entry-side, 2 exit-side; 0 past the count) to root_ptr and {t, p.xyz, normal.xyz} (n x k x 7
    float32) to hit_ptr.  Any pointer may be None, not all four."""
    ctx = prepared.ctx
    ctx._check(lib.rt_multi_hit_rays(ctx._h, prepared._h, int(n), C.c_void_p(rays_ptr), float(t_min), float(t_max), int(k),
                                     C.c_void_p(count_ptr), C.c_void_p(index_ptr), C.c_void_p(root_ptr), C.c_void_p(hit_ptr)))


def multi_hit_rays_ranged_into(rays_ptr, n, prepared, t_min_ptr, t_max_ptr, k, count_ptr, index_ptr, root_ptr=None, hit_ptr=None):
    """multi_hit_rays_into with ray i's own interval (t_min_ptr[i], t_max_ptr[i]) (rt_multi_hit_rays_ranged); a ray whose interval
    fails 0 <= t_min <= t_max <= 1e9 (NaN included) has no crossing."""
    ctx = prepared.ctx
    ctx._check(lib.rt_multi_hit_rays_ranged(ctx._h, prepared._h, int(n), C.c_void_p(rays_ptr), C.c_void_p(t_min_ptr), C.c_void_p(t_max_ptr),
                                            int(k), C.c_void_p(count_ptr), C.c_void_p(index_ptr), C.c_void_p(root_ptr), C.c_void_p(hit_ptr)))


def trace_paths_into(rays_ptr, n, prepared, k, count_ptr=None, end_ptr=None, index_ptr=None, hit_ptr=None, light_ptr=None, last_ray_ptr=None,
                     colour_ptr=None, max_depth=MAX_DEPTH, rays_per_wave=0):
    """Enqueue the mirror-bounce chains of `n` rays (rt_trace_paths; rt_trace_paths_shaped when rays_per_wave is not 0): per ray the number
    of vertices (n int32, not capped at k) to count_ptr, how the chain ended (n uint8: PATH_ESCAPED, PATH_ABSORBED, PATH_TRUNCATED) to end_ptr,
    the first k vertices' sphere indices (n x k int32, -1 past the count) to index_ptr and {t, p.xyz, normal.xyz} (n x k x 7 float32) to
    hit_ptr, and ray_colour's loop variables at exit: light (n x 3), the last ray (n x 6) and the colour (n x 3 float32, rt_trace_rays's).
    Any pointer may be None, not all seven.  rays_per_wave: 0 (the library's rule), or the rays a wave owns, a multiple of 64 in [64, 4096];
    it changes no bit of the answer."""
    ctx = prepared.ctx
    outs = [C.c_void_p(q) for q in (count_ptr, end_ptr, index_ptr, hit_ptr, light_ptr, last_ray_ptr, colour_ptr)]
    if rays_per_wave == 0:
        ctx._check(lib.rt_trace_paths(ctx._h, prepared._h, int(n), C.c_void_p(rays_ptr), int(max_depth), int(k), *outs))
    else:
        ctx._check(lib.rt_trace_paths_shaped(ctx._h, prepared._h, int(n), C.c_void_p(rays_ptr), int(max_depth), int(k), *outs, int(rays_per_wave)))


def nearest_spheres_into(points_ptr, n, prepared, k, count_ptr, index_ptr, gap_ptr=None, max_dist=1e9):
    """Enqueue the proximity query of `n` points (n x 3 float32 at points_ptr; rt_nearest_spheres): per point, the spheres whose gap
    (signed distance from the point to the surface, negative inside) is <= max_dist, ordered by (gap, sphere index): their count
    (n int32, not capped at k) to count_ptr, the first k indices into L (n x k int32, -1 past the count) to index_ptr and their gaps
    (n x k float32, 0 past the count) to gap_ptr.  count_ptr None: k-nearest mode (the walk prunes by the k-th gap; the same slots).
    Any pointer may be None, not all three."""
    ctx = prepared.ctx
    ctx._check(lib.rt_nearest_spheres(ctx._h, prepared._h, int(n), C.c_void_p(points_ptr), float(max_dist), int(k), C.c_void_p(count_ptr),
                                      C.c_void_p(index_ptr), C.c_void_p(gap_ptr)))


def nearest_spheres_ranged_into(points_ptr, n, prepared, max_dist_ptr, k, count_ptr, index_ptr, gap_ptr=None):
    """nearest_spheres_into with point i's own bound max_dist_ptr[i] (n float32 on the device; rt_nearest_spheres_ranged); a bound outside
    [0, 1e9] (NaN, +-inf included) makes its point a miss."""
    ctx = prepared.ctx
    ctx._check(lib.rt_nearest_spheres_ranged(ctx._h, prepared._h, int(n), C.c_void_p(points_ptr), C.c_void_p(max_dist_ptr), int(k),
                                             C.c_void_p(count_ptr), C.c_void_p(index_ptr), C.c_void_p(gap_ptr)))


def spheres_within_count_into(points_ptr, n, prepared, offsets_ptr, max_dist=1e9, max_dist_ptr=None, first_ptr=None):
    """Enqueue the count pass of the range query of `n` points (n x 3 float32 at points_ptr; rt_spheres_within_count): offsets_ptr receives
    n + 1 int64, offsets[i + 1] - offsets[i] = the number of spheres with gap <= the point's bound -- the scalar max_dist, or max_dist_ptr[i]
    (n float32 on the device) -- and index >= first_ptr[i] (n int32 on the device; None: no lower bound).  Asynchronous: read offsets[n] (the
    total) after ctx.sync() or with a copy on the context's stream, then call spheres_within_fill_into with the same arguments."""
    ctx = prepared.ctx
    ctx._check(lib.rt_spheres_within_count(ctx._h, prepared._h, int(n), C.c_void_p(points_ptr), float(max_dist), C.c_void_p(max_dist_ptr),
                                           C.c_void_p(first_ptr), C.c_void_p(offsets_ptr)))


def spheres_within_fill_into(points_ptr, n, prepared, offsets_ptr, capacity, index_ptr, gap_ptr=None, point_ptr=None, max_dist=1e9,
                             max_dist_ptr=None, first_ptr=None):
    """Enqueue the fill pass (rt_spheres_within_fill) for the offsets of spheres_within_count_into on the same points, bounds and scene: row i
    at [offsets[i], offsets[i + 1]) of index_ptr (int32, ascending sphere index into L), gap_ptr (float32) and point_ptr (int32, the row number
    of each entry); `capacity` = the entries each array holds: nothing is written at or past it.  Any pointer may be None, not all three."""
    ctx = prepared.ctx
    ctx._check(lib.rt_spheres_within_fill(ctx._h, prepared._h, int(n), C.c_void_p(points_ptr), float(max_dist), C.c_void_p(max_dist_ptr),
                                          C.c_void_p(first_ptr), C.c_void_p(offsets_ptr), int(capacity), C.c_void_p(index_ptr),
                                          C.c_void_p(gap_ptr), C.c_void_p(point_ptr)))


def spheres_in_boxes_count_into(boxes_ptr, n, prepared, offsets_ptr, margin=0.0, margin_ptr=None, first_ptr=None):
    """Enqueue the count pass of the box query of `n` boxes (n x 6 float32 at boxes_ptr, rows {lo.xyz, hi.xyz}; rt_spheres_in_boxes_count):
    offsets_ptr receives n + 1 int64, offsets[i + 1] - offsets[i] = the number of spheres whose gap to box i is <= the box's margin -- the scalar
    margin, or margin_ptr[i] (n float32 on the device) -- and index >= first_ptr[i] (n int32 on the device; None: no lower bound).
    Asynchronous, as spheres_within_count_into; then call spheres_in_boxes_fill_into with the same arguments."""
    ctx = prepared.ctx
    ctx._check(lib.rt_spheres_in_boxes_count(ctx._h, prepared._h, int(n), C.c_void_p(boxes_ptr), float(margin), C.c_void_p(margin_ptr),
                                             C.c_void_p(first_ptr), C.c_void_p(offsets_ptr)))


def spheres_in_boxes_fill_into(boxes_ptr, n, prepared, offsets_ptr, capacity, index_ptr, gap_ptr=None, point_ptr=None, margin=0.0,
                               margin_ptr=None, first_ptr=None):
    """Enqueue the fill pass (rt_spheres_in_boxes_fill) for the offsets of spheres_in_boxes_count_into on the same boxes, margins and scene:
    the arrays of spheres_within_fill_into (point_ptr: the row, i.e. box, number of each entry); nothing is written at or past `capacity`."""
    ctx = prepared.ctx
    ctx._check(lib.rt_spheres_in_boxes_fill(ctx._h, prepared._h, int(n), C.c_void_p(boxes_ptr), float(margin), C.c_void_p(margin_ptr),
                                            C.c_void_p(first_ptr), C.c_void_p(offsets_ptr), int(capacity), C.c_void_p(index_ptr),
                                            C.c_void_p(gap_ptr), C.c_void_p(point_ptr)))


def spheres_in_planes_count_into(planes_ptr, n, nplanes, prepared, offsets_ptr, margin=0.0, margin_ptr=None, first_ptr=None):
    """Enqueue the count pass of the plane-set query of `n` queries of `nplanes` planes each (n x nplanes x 4 float32 at planes_ptr, rows
    {a, b, c, d}, inside a x + b y + c z + d >= 0; 1 <= nplanes <= 8; rt_spheres_in_planes_count): offsets_ptr receives n + 1 int64,
    offsets[i + 1] - offsets[i] = the number of spheres whose gap to query i's planes is <= the query's margin -- the scalar margin, or
    margin_ptr[i] (n float32 on the device) -- and index >= first_ptr[i] (n int32 on the device; None: no lower bound).  Asynchronous, as
    spheres_in_boxes_count_into; then call spheres_in_planes_fill_into with the same arguments."""
    ctx = prepared.ctx
    ctx._check(lib.rt_spheres_in_planes_count(ctx._h, prepared._h, int(n), C.c_void_p(planes_ptr), int(nplanes), float(margin),
                                              C.c_void_p(margin_ptr), C.c_void_p(first_ptr), C.c_void_p(offsets_ptr)))


def spheres_in_planes_fill_into(planes_ptr, n, nplanes, prepared, offsets_ptr, capacity, index_ptr, gap_ptr=None, point_ptr=None, margin=0.0,
                                margin_ptr=None, first_ptr=None):
    """Enqueue the fill pass (rt_spheres_in_planes_fill) for the offsets of spheres_in_planes_count_into on the same planes, margins and
    scene: the arrays of spheres_in_boxes_fill_into (point_ptr: the row, i.e. query, number of each entry); nothing is written at or past
    `capacity`."""
    ctx = prepared.ctx
    ctx._check(lib.rt_spheres_in_planes_fill(ctx._h, prepared._h, int(n), C.c_void_p(planes_ptr), int(nplanes), float(margin),
                                             C.c_void_p(margin_ptr), C.c_void_p(first_ptr), C.c_void_p(offsets_ptr), int(capacity),
                                             C.c_void_p(index_ptr), C.c_void_p(gap_ptr), C.c_void_p(point_ptr)))


def contact_pairs_count_into(prepared, offsets_ptr, margin=0.0):
    """Enqueue the count pass of the scene's contact pairs (rt_contact_pairs_count): offsets_ptr receives num_spheres + 1 int64, row i counting
    the j > i with gap(centre_i, L[j]) <= radius_i + margin.  Asynchronous, as spheres_within_count_into."""
    ctx = prepared.ctx
    ctx._check(lib.rt_contact_pairs_count(ctx._h, prepared._h, float(margin), C.c_void_p(offsets_ptr)))


def contact_pairs_fill_into(prepared, offsets_ptr, capacity, pair_ptr, gap_ptr=None, margin=0.0):
    """Enqueue the fill pass of the contact pairs (rt_contact_pairs_fill): pair_ptr receives total x 2 int32, rows (i, j) with i < j in
    ascending (i, j), indices into L; gap_ptr total float32, the gap from centre i to the surface of j.  Either may be None, not both."""
    ctx = prepared.ctx
    ctx._check(lib.rt_contact_pairs_fill(ctx._h, prepared._h, float(margin), C.c_void_p(offsets_ptr), int(capacity), C.c_void_p(pair_ptr),
                                         C.c_void_p(gap_ptr)))


def contact_clusters_into(prepared, root_ptr, cluster_ptr=None, size_ptr=None, num_ptr=None, margin=0.0):
    """Enqueue the connected components of the contact pairs' graph at `margin` (rt_contact_clusters): root_ptr receives num_spheres int32,
    root[i] = the smallest index in i's component; cluster_ptr num_spheres int32, dense ids in ascending order of the root; size_ptr
    num_spheres int32, the size of i's cluster; num_ptr one int64, the number of clusters.  All but root_ptr may be None.  Indices are into L
    (Morton order): prepared.sphere_ids() maps them to the caller's order.  Asynchronous, as contact_pairs_count_into."""
    ctx = prepared.ctx
    ctx._check(lib.rt_contact_clusters(ctx._h, prepared._h, float(margin), C.c_void_p(root_ptr), C.c_void_p(cluster_ptr), C.c_void_p(size_ptr),
                                       C.c_void_p(num_ptr)))


def sweep_spheres_into(rays_ptr, n, prepared, radius, k, count_ptr, index_ptr, start_ptr=None, hit_ptr=None, t_min=0.0, t_max=1.0):
    """Enqueue the first k (1 <= k <= 32) contacts of `n` moving spheres of radius `radius` (rt_sweep_spheres): ray i is the centre's
    origin and its displacement per unit t, the contacts over (t_min, t_max) are ordered by (tau, sphere).  Their count (n int32, not capped
    at k) to count_ptr, sphere indices (n x k int32, -1 past the count) to index_ptr, start flags (n x k uint8: 1 for an overlap where the
    interval begins, tau = t_min) to start_ptr and {tau, centre at contact xyz, normal xyz} (n x k x 7 float32) to hit_ptr.  Any pointer may
    be None, not all four."""
    ctx = prepared.ctx
    ctx._check(lib.rt_sweep_spheres(ctx._h, prepared._h, int(n), C.c_void_p(rays_ptr), float(radius), float(t_min), float(t_max), int(k),
                                    C.c_void_p(count_ptr), C.c_void_p(index_ptr), C.c_void_p(start_ptr), C.c_void_p(hit_ptr)))


def sweep_spheres_ranged_into(rays_ptr, n, prepared, radius_ptr, t_min_ptr, t_max_ptr, k, count_ptr, index_ptr, start_ptr=None, hit_ptr=None,
                              exclude_ptr=None):
    """sweep_spheres_into with query i's own radius_ptr[i] and interval (t_min_ptr[i], t_max_ptr[i]) (rt_sweep_spheres_ranged; n float32
    each): a query whose interval fails 0 <= t_min <= t_max <= 1e9 or whose radius fails 0 <= radius <= 1e9 (NaN included) has no contact.
    exclude_ptr: None, or n int32 on the device -- sphere exclude_ptr[i] is skipped for query i (a scene sweeping its own spheres)."""
    ctx = prepared.ctx
    ctx._check(lib.rt_sweep_spheres_ranged(ctx._h, prepared._h, int(n), C.c_void_p(rays_ptr), C.c_void_p(radius_ptr), C.c_void_p(t_min_ptr),
                                           C.c_void_p(t_max_ptr), C.c_void_p(exclude_ptr), int(k), C.c_void_p(count_ptr),
                                           C.c_void_p(index_ptr), C.c_void_p(start_ptr), C.c_void_p(hit_ptr)))


def spheres_along_rays_count_into(rays_ptr, n, prepared, offsets_ptr, radius=0.0, t_min=0.0, t_max=1e9, radius_ptr=None, t_min_ptr=None,
                                  t_max_ptr=None, exclude_ptr=None, first_ptr=None):
    """Enqueue the count pass of the along-ray query of `n` queries (n x 6 float32 at rays_ptr; rt_spheres_along_rays_count): offsets_ptr
    receives n + 1 int64, offsets[i + 1] - offsets[i] = the number of spheres the moving sphere of query i touches over its interval -- every
    contact sweep_spheres would count -- with index != exclude_ptr[i] and index >= first_ptr[i] (n int32 each on the device; None: no such
    filter).  radius_ptr: None (the scalar radius for every query) or n float32 on the device; t_min_ptr / t_max_ptr: both None (the scalar
    pair) or both n float32 on the device.  Asynchronous, as spheres_within_count_into; then call spheres_along_rays_fill_into with the same
    arguments."""
    ctx = prepared.ctx
    ctx._check(lib.rt_spheres_along_rays_count(ctx._h, prepared._h, int(n), C.c_void_p(rays_ptr), float(radius), C.c_void_p(radius_ptr),
                                               float(t_min), float(t_max), C.c_void_p(t_min_ptr), C.c_void_p(t_max_ptr),
                                               C.c_void_p(exclude_ptr), C.c_void_p(first_ptr), C.c_void_p(offsets_ptr)))


def spheres_along_rays_fill_into(rays_ptr, n, prepared, offsets_ptr, capacity, index_ptr, roots_ptr=None, start_ptr=None, query_ptr=None,
                                 radius=0.0, t_min=0.0, t_max=1e9, radius_ptr=None, t_min_ptr=None, t_max_ptr=None, exclude_ptr=None,
                                 first_ptr=None):
    """Enqueue the fill pass (rt_spheres_along_rays_fill) for the offsets of spheres_along_rays_count_into on the same queries and scene: row
    i at [offsets[i], offsets[i + 1]) of index_ptr (int32, ascending sphere index into L), roots_ptr (rows of two float32: the unclamped roots
    t1, t2 against the sphere widened by the query's radius), start_ptr (uint8: 1 for an overlap where the interval begins) and query_ptr
    (int32, the row number of each entry); `capacity` = the entries each array holds: nothing is written at or past it.  Any pointer may be
    None, not all four."""
    ctx = prepared.ctx
    ctx._check(lib.rt_spheres_along_rays_fill(ctx._h, prepared._h, int(n), C.c_void_p(rays_ptr), float(radius), C.c_void_p(radius_ptr),
                                              float(t_min), float(t_max), C.c_void_p(t_min_ptr), C.c_void_p(t_max_ptr),
                                              C.c_void_p(exclude_ptr), C.c_void_p(first_ptr), C.c_void_p(offsets_ptr), int(capacity),
                                              C.c_void_p(index_ptr), C.c_void_p(roots_ptr), C.c_void_p(start_ptr), C.c_void_p(query_ptr)))


def visible_pairs_into(points_ptr, n, targets_ptr, m, prepared, mode, visible_ptr=None, count_ptr=None, t_min=0.0, t_max=1e9, words_per_wave=0):
    """Enqueue the visibility matrix of `n` points (n x 3 float32 at points_ptr) against `m` targets or directions (m x 3 float32 at
    targets_ptr; mode PAIRS_TARGETS: the ray of pair (i, j) is o = P_i, d = T_j - P_i; PAIRS_DIRECTIONS: d = T_j) over (t_min, t_max)
    (rt_visible_pairs; rt_visible_pairs_shaped when words_per_wave is not 0): n x W uint64 words, W = (m + 63) // 64, to visible_ptr -- bit
    j & 63 of word [i, j >> 6] is 1 iff the pair's ray is valid and occluded_rays answers False for it -- and the set bits of each row
    (n int32) to count_ptr.  Either pointer may be None, not both.  words_per_wave: 0 (the library's rule), or the consecutive words of a
    row that one wave owns; it changes no bit of the answer.  Asynchronous: ctx.sync() completes it."""
    ctx = prepared.ctx
    args = (ctx._h, prepared._h, int(n), C.c_void_p(points_ptr), int(m), C.c_void_p(targets_ptr), int(mode), float(t_min), float(t_max),
            C.c_void_p(visible_ptr), C.c_void_p(count_ptr))
    if words_per_wave == 0:
        ctx._check(lib.rt_visible_pairs(*args))
    else:
        ctx._check(lib.rt_visible_pairs_shaped(*args, int(words_per_wave)))


def camera_rays_into(rays_ptr, h, w, prepared, cam=None):
    """Enqueue the h * w primary rays rt_render_image would trace (rt_camera_rays) into rays_ptr (h * w x 6 float32)."""
    ctx = prepared.ctx
    c = None
    if cam is not None:
        c = np.ascontiguousarray(cam, dtype=np.float32)
        assert c.size == 12
    ctx._check(lib.rt_camera_rays(ctx._h, prepared._h, int(h), int(w), None if c is None else c.ctypes.data, C.c_void_p(rays_ptr)))


class _Scope:
    """The device buffers of one query call: whatever alloc() and upload() hand out is freed when the `with` block is left, on every path."""

    def __init__(self, ctx):
        self.ctx, self._bufs = ctx, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for buf in self._bufs:
            buf.free()
        return False

    def alloc(self, nbytes):
        buf = DeviceBuffer(self.ctx, max(nbytes, 4))
        self._bufs.append(buf)
        return buf

    def upload(self, a):
        """The device pointer of a copy of the contiguous numpy array `a`."""
        buf = self.alloc(a.nbytes)
        if a.nbytes:
            self.ctx._check(lib.rt_copy_to_device(self.ctx._h, C.c_void_p(buf.ptr), a.ctypes.data, a.nbytes))
        return buf.ptr


def _check_tensor(t, dev, dtype, name):
    if str(t.dtype) != f"torch.{dtype}" or not t.is_contiguous() or t.device.type != "cuda" or t.device.index != dev:
        raise ValueError(f"{name}: a contiguous {dtype} tensor on cuda:{dev} is required")


_RAYS = ("rays", 6, "rays must be (n, 6): origin.xyz, dir.xyz")
_POINTS = ("points", 3, "points must be (n, 3)")
_BOXES = ("boxes", 6, "boxes must be (n, 6): lo.xyz, hi.xyz")


def _device_rows(scope, rows, name, cols, shape_error):
    """(pointer, n) for `rows` (n x cols float32; _RAYS, _POINTS): a numpy array is uploaded to a buffer of the scope; a contiguous float32
    torch tensor on the context's device is used in place."""
    if hasattr(rows, "data_ptr"):
        _check_tensor(rows, scope.ctx.device_info()["device"], "float32", name)
        if rows.dim() != 2 or rows.shape[1] != cols:
            raise ValueError(shape_error)
        return rows.data_ptr(), int(rows.shape[0])
    a = np.ascontiguousarray(rows, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != cols:
        raise ValueError(shape_error)
    return scope.upload(a), a.shape[0]


def _is_bound_array(b):
    return hasattr(b, "data_ptr") or np.ndim(b) > 0


def _device_values(scope, dev, n, name, v, dtype, kind, what, per, convert):
    """The device pointer of the (n,) per-query values `v`: a contiguous `dtype` torch tensor on the context's device is used in place; a numpy
    array of dtype kind `kind` is passed through convert() and uploaded to a buffer of the scope."""
    if hasattr(v, "data_ptr"):
        _check_tensor(v, dev, dtype, name)
        if v.dim() != 1 or v.shape[0] != n:
            raise ValueError(f"{name} must be ({n},), one {what} per {per}; got {tuple(v.shape)}")
        return v.data_ptr()
    a = np.asarray(v)
    if not np.issubdtype(a.dtype, kind):
        raise ValueError(f"{name}: {'a floating-point' if kind is np.floating else 'an integer'} array is required; got {a.dtype}")
    if a.shape != (n,):
        raise ValueError(f"{name} must be ({n},), one {what} per {per}; got {a.shape}")
    return scope.upload(convert(a))


def _device_bound(scope, dev, n, name, b, per="ray"):
    """The device pointer of one bound of the ranged entries: an (n,) array -- numpy (a floating dtype, uploaded as float32) or a contiguous
    float32 torch tensor on the context's device (used in place) -- or a scalar, checked by the scalar entries' rule and broadcast."""
    if _is_bound_array(b):
        return _device_values(scope, dev, n, name, b, "float32", np.floating, "bound", per, lambda a: np.ascontiguousarray(a, dtype=np.float32))
    v = np.float32(b)
    if not (np.isfinite(v) and 0.0 <= v <= 1e9):
        raise RtError(f"{name} = {b!r}: a scalar bound must be finite and in [0, 1e9]")
    return scope.upload(np.full(n, v, dtype=np.float32))


def _device_bounds(scope, n, t_min, t_max):
    """(t_min pointer, t_max pointer) of the ranged ray entries (_device_bound)."""
    dev = scope.ctx.device_info()["device"]
    return _device_bound(scope, dev, n, "t_min", t_min), _device_bound(scope, dev, n, "t_max", t_max)


def _device_first(scope, dev, n, first, name="first", per="point"):
    """The device pointer of the per-point lower index bounds `first` (or, as `name`, the sweep queries' excluded indices): an (n,) integer
    numpy array (uploaded as int32, clipped to int32's range first) or a contiguous int32 torch tensor on the context's device (used in
    place)."""
    return _device_values(scope, dev, n, name, first, "int32", np.integer, "index", per,
                          lambda a: np.ascontiguousarray(np.clip(a, -2 ** 31, 2 ** 31 - 1), dtype=np.int32))


def _device_words(scope, v, name, n):
    """(pointer, count) of a vector of 32-bit words (sphere groups, per-query masks): an integer numpy array with values in [0, 2^32) is
    uploaded as uint32; a contiguous int32 or uint32 torch tensor on the context's device is used in place, its bits being the words.
    n: the length it must have (None: any)."""
    if hasattr(v, "data_ptr"):
        dev = scope.ctx.device_info()["device"]
        if str(v.dtype) not in ("torch.int32", "torch.uint32") or not v.is_contiguous() or v.device.type != "cuda" or v.device.index != dev:
            raise ValueError(f"{name}: a contiguous int32 or uint32 tensor on cuda:{dev} is required")
        if v.dim() != 1 or (n is not None and v.shape[0] != n):
            raise ValueError(f"{name} must be ({'n' if n is None else n},); got {tuple(v.shape)}")
        return v.data_ptr(), int(v.shape[0])
    a = np.asarray(v)
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name}: an integer array is required; got {a.dtype}")
    if a.ndim != 1 or (n is not None and a.shape[0] != n):
        raise ValueError(f"{name} must be ({'n' if n is None else n},); got {a.shape}")
    if a.size and (int(a.min()) < 0 or int(a.max()) >= 2 ** 32):
        raise ValueError(f"{name}: values must be in [0, 2^32)")
    return scope.upload(np.ascontiguousarray(a.astype(np.uint32))), int(a.shape[0])


def _mask_args(scope, n, mask):
    """(scalar mask, mask pointer or None) of the mask= keyword: a Python int in [0, 2^32) is the scalar mask of every query; an (n,) integer
    array or int32 / uint32 device tensor is one mask per query."""
    if _is_bound_array(mask):
        return 0, _device_words(scope, mask, "mask", n)[0]
    m = int(mask)
    if not 0 <= m < 2 ** 32:
        raise ValueError(f"mask = {mask!r}: a scalar mask must be in [0, 2^32)")
    return m, None


def intersect_rays_masked_into(rays_ptr, n, prepared, index_ptr, hit_ptr=None, t_min=0.0, t_max=1e9, t_min_ptr=None, t_max_ptr=None, mask=0xFFFFFFFF,
                               mask_ptr=None):
    """intersect_rays_into over the spheres the mask sees (rt_intersect_rays_masked; Prepared.set_groups): sphere j is seen iff groups[j] &
    mask != 0 -- the scalar `mask`, or mask_ptr[i] (n uint32 on the device) for ray i.  t_min_ptr / t_max_ptr: both None (the scalar interval)
    or both given (n float32 each, the scalars are ignored)."""
    ctx = prepared.ctx
    ctx._check(lib.rt_intersect_rays_masked(ctx._h, prepared._h, int(n), C.c_void_p(rays_ptr), float(t_min), float(t_max), C.c_void_p(t_min_ptr),
                                            C.c_void_p(t_max_ptr), int(mask), C.c_void_p(mask_ptr), C.c_void_p(index_ptr), C.c_void_p(hit_ptr)))


def occluded_rays_masked_into(rays_ptr, n, prepared, out_ptr, t_min=0.0, t_max=1e9, t_min_ptr=None, t_max_ptr=None, mask=0xFFFFFFFF, mask_ptr=None):
    """occluded_rays_into over the spheres the mask sees (rt_occluded_rays_masked); arguments as intersect_rays_masked_into."""
    ctx = prepared.ctx
    ctx._check(lib.rt_occluded_rays_masked(ctx._h, prepared._h, int(n), C.c_void_p(rays_ptr), float(t_min), float(t_max), C.c_void_p(t_min_ptr),
                                           C.c_void_p(t_max_ptr), int(mask), C.c_void_p(mask_ptr), C.c_void_p(out_ptr)))


def nearest_spheres_masked_into(points_ptr, n, prepared, k, count_ptr, index_ptr, gap_ptr=None, max_dist=1e9, max_dist_ptr=None, mask=0xFFFFFFFF,
                                mask_ptr=None):
    """nearest_spheres_into over the spheres the mask sees (rt_nearest_spheres_masked): the scalar `mask`, or mask_ptr[i] (n uint32 on the
    device) for point i; max_dist_ptr: None (the scalar bound) or n float32 on the device (the scalar is ignored)."""
    ctx = prepared.ctx
    ctx._check(lib.rt_nearest_spheres_masked(ctx._h, prepared._h, int(n), C.c_void_p(points_ptr), float(max_dist), C.c_void_p(max_dist_ptr),
                                             int(mask), C.c_void_p(mask_ptr), int(k), C.c_void_p(count_ptr), C.c_void_p(index_ptr),
                                             C.c_void_p(gap_ptr)))


def spheres_within_masked_count_into(points_ptr, n, prepared, offsets_ptr, max_dist=1e9, max_dist_ptr=None, first_ptr=None, mask=0xFFFFFFFF,
                                     mask_ptr=None):
    """spheres_within_count_into over the spheres the mask sees (rt_spheres_within_masked_count): the scalar `mask`, or mask_ptr[i] (n uint32
    on the device) for point i."""
    ctx = prepared.ctx
    ctx._check(lib.rt_spheres_within_masked_count(ctx._h, prepared._h, int(n), C.c_void_p(points_ptr), float(max_dist), C.c_void_p(max_dist_ptr),
                                                  int(mask), C.c_void_p(mask_ptr), C.c_void_p(first_ptr), C.c_void_p(offsets_ptr)))


def spheres_within_masked_fill_into(points_ptr, n, prepared, offsets_ptr, capacity, index_ptr, gap_ptr=None, point_ptr=None, max_dist=1e9,
                                    max_dist_ptr=None, first_ptr=None, mask=0xFFFFFFFF, mask_ptr=None):
    """spheres_within_fill_into for the offsets of spheres_within_masked_count_into on the same points, bounds, masks and scene
    (rt_spheres_within_masked_fill)."""
    ctx = prepared.ctx
    ctx._check(lib.rt_spheres_within_masked_fill(ctx._h, prepared._h, int(n), C.c_void_p(points_ptr), float(max_dist), C.c_void_p(max_dist_ptr),
                                                 int(mask), C.c_void_p(mask_ptr), C.c_void_p(first_ptr), C.c_void_p(offsets_ptr), int(capacity),
                                                 C.c_void_p(index_ptr), C.c_void_p(gap_ptr), C.c_void_p(point_ptr)))


def trace_rays(prepared, rays, max_depth=MAX_DEPTH):
    """ray_colour of every ray (ray.fut:126-148) -> (colour (n, 3) float32, pixel (n,) int32) numpy arrays."""
    with _Scope(prepared.ctx) as s:
        ptr, n = _device_rows(s, rays, *_RAYS)
        col, px = s.alloc(12 * n), s.alloc(4 * n)
        trace_rays_into(ptr, n, prepared, col.ptr, px.ptr, max_depth)
        return col.to_host((n, 3), np.float32), px.to_host((n,))


def intersect_rays(prepared, rays, t_min=0.0, t_max=1e9, mask=None):
    """objs_hit bvh r t_min t_max of every ray (ray.fut:76-86) -> (index (n,) int32, hit (n, 7) float32) numpy arrays.
    Either bound may be an (n,) array, one per ray (rt_intersect_rays_ranged; a scalar next to it is broadcast).
    mask: None (the default: every sphere, the unmasked entry), or -- on a scene with Prepared.set_groups -- a Python int, the mask of every
    ray, or an (n,) integer array / int32 or uint32 device tensor, one mask per ray (rt_intersect_rays_masked): sphere j is seen iff groups[j] & mask != 0;
    indices still are indices into the whole of L."""
    ranged = _is_bound_array(t_min) or _is_bound_array(t_max)
    with _Scope(prepared.ctx) as s:
        ptr, n = _device_rows(s, rays, *_RAYS)
        if ranged:
            lo_ptr, hi_ptr = _device_bounds(s, n, t_min, t_max)
        idx, hit = s.alloc(4 * n), s.alloc(28 * n)
        if mask is not None:
            m, m_ptr = _mask_args(s, n, mask)
            if ranged:
                intersect_rays_masked_into(ptr, n, prepared, idx.ptr, hit.ptr, 0.0, 0.0, lo_ptr, hi_ptr, m, m_ptr)
            else:
                intersect_rays_masked_into(ptr, n, prepared, idx.ptr, hit.ptr, t_min, t_max, None, None, m, m_ptr)
        elif ranged:
            intersect_rays_ranged_into(ptr, n, prepared, lo_ptr, hi_ptr, idx.ptr, hit.ptr)
        else:
            intersect_rays_into(ptr, n, prepared, idx.ptr, hit.ptr, t_min, t_max)
        return idx.to_host((n,)), hit.to_host((n, 7), np.float32)


def occluded_rays(prepared, rays, t_min=0.0, t_max=1e9, mask=None):
    """Occlusion of every ray over (t_min, t_max) (rt_occluded_rays) -> (n,) bool numpy array.  Either bound may be an (n,)
    array, one per ray (rt_occluded_rays_ranged; a scalar next to it is broadcast).
    mask: None (the default: every sphere, the unmasked entry), or -- on a scene with Prepared.set_groups -- a Python int, the mask of every
    ray, or an (n,) integer array / int32 or uint32 device tensor, one mask per ray (rt_occluded_rays_masked): sphere j is seen iff groups[j] & mask != 0;
    indices still are indices into the whole of L."""
    ranged = _is_bound_array(t_min) or _is_bound_array(t_max)
    with _Scope(prepared.ctx) as s:
        ptr, n = _device_rows(s, rays, *_RAYS)
        if ranged:
            lo_ptr, hi_ptr = _device_bounds(s, n, t_min, t_max)
        out = s.alloc(n)
        if mask is not None:
            m, m_ptr = _mask_args(s, n, mask)
            if ranged:
                occluded_rays_masked_into(ptr, n, prepared, out.ptr, 0.0, 0.0, lo_ptr, hi_ptr, m, m_ptr)
            else:
                occluded_rays_masked_into(ptr, n, prepared, out.ptr, t_min, t_max, None, None, m, m_ptr)
        elif ranged:
            occluded_rays_ranged_into(ptr, n, prepared, lo_ptr, hi_ptr, out.ptr)
        else:
            occluded_rays_into(ptr, n, prepared, out.ptr, t_min, t_max)
        return out.to_host((n,), np.uint8).astype(bool)


def multi_hit_rays(prepared, rays, k, t_min=0.0, t_max=1e9):
    """The first k sphere crossings of every ray over (t_min, t_max) (rt_multi_hit_rays) -> (count (n,) int32, index (n, k) int32,
    root (n, k) uint8, hit (n, k, 7) float32) numpy arrays.  Either bound may be an (n,) array, one per ray (rt_multi_hit_rays_ranged;
    a scalar next to it is broadcast)."""
    k = int(k)
    ranged = _is_bound_array(t_min) or _is_bound_array(t_max)
    with _Scope(prepared.ctx) as s:
        ptr, n = _device_rows(s, rays, *_RAYS)
        if ranged:
            lo_ptr, hi_ptr = _device_bounds(s, n, t_min, t_max)
        nk = n * max(k, 0)
        cnt, idx, root, hit = s.alloc(4 * n), s.alloc(4 * nk), s.alloc(nk), s.alloc(28 * nk)
        if ranged:
            multi_hit_rays_ranged_into(ptr, n, prepared, lo_ptr, hi_ptr, k, cnt.ptr, idx.ptr, root.ptr, hit.ptr)
        else:
            multi_hit_rays_into(ptr, n, prepared, k, cnt.ptr, idx.ptr, root.ptr, hit.ptr, t_min, t_max)
        return (cnt.to_host((n,)), idx.to_host((n, k)), root.to_host((n, k), np.uint8), hit.to_host((n, k, 7), np.float32))


def sweep_spheres(prepared, rays, radius, k=1, t_min=0.0, t_max=1.0, exclude=None):
    """The first k contacts of a sphere of radius `radius` whose centre moves from rays[i, :3] by rays[i, 3:] per unit t, over (t_min, t_max)
    (rt_sweep_spheres) -> (count (n,) int32, index (n, k) int32, start (n, k) uint8, hit (n, k, 7) float32) numpy arrays.  With the default
    t_max = 1.0 the direction is the displacement of one step.  A contact is the first touch of a scene sphere (start 0, tau = the time of
    touch) or an overlap that already exists where the interval begins (start 1, tau = t_min); they are ordered by (tau, index).  hit =
    {tau, the moving centre at contact, the normal from the scene sphere's centre towards it}.  k = 1 is the classic sphere cast.
    radius, t_min or t_max may be an (n,) array / device tensor, one per query (rt_sweep_spheres_ranged; a scalar next to it is broadcast;
    an invalid array value makes its query a miss; an invalid scalar, or a scalar pair with t_min > t_max, is an RtError).  exclude: None,
    or an (n,) integer array / int32 device tensor -- sphere exclude[i] of L is skipped for query i, so a scene can sweep its own spheres
    (also the ranged entry)."""
    k = int(k)
    ranged = _is_bound_array(radius) or _is_bound_array(t_min) or _is_bound_array(t_max) or exclude is not None
    with _Scope(prepared.ctx) as s:
        ptr, n = _device_rows(s, rays, *_RAYS)
        if ranged:
            dev = s.ctx.device_info()["device"]
            # (a scalar pair is held to the scalar entry's rule as a pair: each scalar alone passes _device_bound with t_min > t_max)
            if not _is_bound_array(t_min) and not _is_bound_array(t_max) and not np.float32(t_min) <= np.float32(t_max):
                raise RtError(f"t_min = {t_min!r}, t_max = {t_max!r}: scalar bounds must satisfy t_min <= t_max")
            rad_ptr = _device_bound(s, dev, n, "radius", radius, per="query")
            lo_ptr = _device_bound(s, dev, n, "t_min", t_min, per="query")
            hi_ptr = _device_bound(s, dev, n, "t_max", t_max, per="query")
            ex_ptr = _device_first(s, dev, n, exclude, name="exclude", per="query") if exclude is not None else None
        nk = n * max(k, 0)
        cnt, idx, start, hit = s.alloc(4 * n), s.alloc(4 * nk), s.alloc(nk), s.alloc(28 * nk)
        if ranged:
            sweep_spheres_ranged_into(ptr, n, prepared, rad_ptr, lo_ptr, hi_ptr, k, cnt.ptr, idx.ptr, start.ptr, hit.ptr, ex_ptr)
        else:
            sweep_spheres_into(ptr, n, prepared, radius, k, cnt.ptr, idx.ptr, start.ptr, hit.ptr, t_min, t_max)
        return (cnt.to_host((n,)), idx.to_host((n, k)), start.to_host((n, k), np.uint8), hit.to_host((n, k, 7), np.float32))


def trace_paths(prepared, rays, k, max_depth=MAX_DEPTH, rays_per_wave=0):
    """The mirror-bounce chain of every ray (rt_trace_paths): ray_colour's loop (ray.fut:126-148) with its vertices kept -> (count (n,) int32,
    end (n,) uint8, index (n, k) int32, hit (n, k, 7) float32, light (n, 3), last_ray (n, 6), colour (n, 3) float32) numpy arrays.  Vertex s
    of a ray is what intersect_rays(0, 1e9) gives for the chain's s-th ray; count is not capped at k; end is PATH_ESCAPED, PATH_ABSORBED or
    PATH_TRUNCATED; light, last_ray and colour are the loop's variables at exit (colour: trace_rays's).  rays: an (n, 6) numpy array, or a
    float32 device tensor used in place."""
    k = int(k)
    with _Scope(prepared.ctx) as s:
        ptr, n = _device_rows(s, rays, *_RAYS)
        nk = n * max(k, 0)
        cnt, end, idx, hit = s.alloc(4 * n), s.alloc(n), s.alloc(4 * nk), s.alloc(28 * nk)
        light, last, col = s.alloc(12 * n), s.alloc(24 * n), s.alloc(12 * n)
        trace_paths_into(ptr, n, prepared, k, cnt.ptr, end.ptr, idx.ptr, hit.ptr, light.ptr, last.ptr, col.ptr, max_depth, rays_per_wave)
        return (cnt.to_host((n,)), end.to_host((n,), np.uint8), idx.to_host((n, k)), hit.to_host((n, k, 7), np.float32),
                light.to_host((n, 3), np.float32), last.to_host((n, 6), np.float32), col.to_host((n, 3), np.float32))


def nearest_spheres(prepared, points, k, max_dist=1e9, count=True):
    """The k nearest spheres of every point (rt_nearest_spheres) -> (count (n,) int32 or None, index (n, k) int32, gap (n, k) float32)
    numpy arrays.  A sphere is selected for point p iff its gap -- sqrtf(|p - c|^2) - r in float32, the signed distance to its surface,
    negative inside -- is <= max_dist; the selected ones are ordered by (gap, index), index being the sphere's place in L (Morton order:
    prepared.sphere_ids() maps it to the caller's order).  `count` is the number selected, not capped at k; slots past it are -1 / 0.0.
    max_dist: a scalar in [0, 1e9], or an (n,) array / device tensor, one bound per point (rt_nearest_spheres_ranged; an invalid bound makes
    its point a miss).  count=False: k-nearest mode -- the walk also prunes by the k-th gap found so far, no count is returned, the slots are
    the same.  `points`: (n, 3) float32, a numpy array or a device tensor.  A point with a non-finite component selects nothing.
    Contacts: the spheres a sphere (c, r) overlaps or touches are those selected at p = c with max_dist = r; for a scene's self-contacts pass
    its own centres and radii -- every sphere finds itself at gap -r.
    nearest_spheres_masked: the same over the spheres a group mask sees."""
    return _nearest_spheres(prepared, points, k, max_dist, count, None)


def nearest_spheres_masked(prepared, points, k, max_dist=1e9, count=True, *, mask):
    """nearest_spheres over the spheres the mask sees (rt_nearest_spheres_masked; the scene needs Prepared.set_groups): sphere j is seen iff
    groups[j] & mask != 0.  mask: a Python int, the mask of every point, or an (n,) integer array / int32 or uint32 device tensor, one mask per
    point (a required keyword).  Everything else as nearest_spheres; indices still are indices into the whole of L."""
    return _nearest_spheres(prepared, points, k, max_dist, count, mask)


def _nearest_spheres(prepared, points, k, max_dist, count, mask):
    k = int(k)
    ranged = _is_bound_array(max_dist)
    with _Scope(prepared.ctx) as s:
        ptr, n = _device_rows(s, points, *_POINTS)
        if ranged:
            md_ptr = _device_bound(s, s.ctx.device_info()["device"], n, "max_dist", max_dist, per="point")
        nk = n * max(k, 0)
        cnt = s.alloc(4 * n) if count else None
        idx, gap = s.alloc(4 * nk), s.alloc(4 * nk)
        cptr = cnt.ptr if cnt is not None else None
        if mask is not None:
            m, m_ptr = _mask_args(s, n, mask)
            nearest_spheres_masked_into(ptr, n, prepared, k, cptr, idx.ptr, gap.ptr, 0.0 if ranged else max_dist, md_ptr if ranged else None, m, m_ptr)
        elif ranged:
            nearest_spheres_ranged_into(ptr, n, prepared, md_ptr, k, cptr, idx.ptr, gap.ptr)
        else:
            nearest_spheres_into(ptr, n, prepared, k, cptr, idx.ptr, gap.ptr, max_dist)
        return (cnt.to_host((n,)) if cnt is not None else None, idx.to_host((n, k)), gap.to_host((n, k), np.float32))


def _csr_query(scope, n, count, fill, columns):
    """The two passes of a CSR query of n rows -> (offsets (n + 1,) int64, one numpy array per column).  count(offsets pointer) runs the count
    pass, fill(offsets pointer, total, a pointer or None per column) the fill pass -- not called when no row has an entry.  columns: (dtype,
    width, want) per entry array, in fill's order and the result's: want True gives (total,) of dtype, (total, width) for width > 1; False
    gives None in its place; None leaves it out of the result."""
    off = scope.alloc(8 * (n + 1))
    count(off.ptr)
    offsets = off.to_host((n + 1,), np.int64)
    total = int(offsets[n])
    bufs = [scope.alloc(np.dtype(dtype).itemsize * width * total) if want else None for dtype, width, want in columns]
    if total:
        fill(off.ptr, total, *(b.ptr if b else None for b in bufs))
    return (offsets,) + tuple(b.to_host((total,) if width == 1 else (total, width), dtype) if b else None
                              for b, (dtype, width, want) in zip(bufs, columns) if want is not None)


def _gap_columns(gaps, rows):
    """The columns of the range, box and plane-set queries: index, gap (optional), and with `rows` the row number of every entry."""
    return (np.int32, 1, True), (np.float32, 1, bool(gaps)), (np.int32, 1, True if rows else None)


def spheres_within(prepared, points, max_dist, first=None, gaps=True, rows=False):
    """EVERY sphere within max_dist of every point (rt_spheres_within_count / _fill), with no cap, in CSR form -> (offsets (n + 1,) int64,
    index (total,) int32, gap (total,) float32 or None[, point (total,) int32]) numpy arrays.  The selection rule is nearest_spheres's: sphere
    j is selected for point i iff its gap -- sqrtf(|p - c|^2) - r in float32 -- is <= the point's bound.  Row i is
    index[offsets[i]:offsets[i + 1]], in ASCENDING sphere index (an index into L, Morton order: prepared.sphere_ids() maps it to the caller's
    order), not by gap: sort a row by (gap, index) to get nearest_spheres's order.  max_dist: a scalar in [0, 1e9], or an (n,) array / device
    tensor, one bound per point (an invalid bound gives an empty row).  first: None, or an (n,) integer array / int32 device tensor: only
    spheres with index >= first[i] are selected for point i.  gaps=False: no gap array (None is returned in its place).  rows=True: also
    `point`, the row number of every entry, so that (point, index) is the list of pairs.  `points`: (n, 3) float32, a numpy array or a device
    tensor.  A point with a non-finite component has an empty row.
    spheres_within_masked: the same over the spheres a group mask sees."""
    return _spheres_within(prepared, points, max_dist, first, gaps, rows, None)


def spheres_within_masked(prepared, points, max_dist, first=None, gaps=True, rows=False, *, mask):
    """spheres_within over the spheres the mask sees (rt_spheres_within_masked_count / _fill; the scene needs Prepared.set_groups): sphere j
    is seen iff groups[j] & mask != 0.  mask: a Python int, the mask of every point, or an (n,) integer array / int32 or uint32 device tensor,
    one mask per point (a required keyword).  Everything else as spheres_within; indices still are indices into the whole of L."""
    return _spheres_within(prepared, points, max_dist, first, gaps, rows, mask)


def _spheres_within(prepared, points, max_dist, first, gaps, rows, mask):
    ranged = _is_bound_array(max_dist)
    with _Scope(prepared.ctx) as s:
        ptr, n = _device_rows(s, points, *_POINTS)
        dev = s.ctx.device_info()["device"]
        md_ptr = _device_bound(s, dev, n, "max_dist", max_dist, per="point") if ranged else None
        md = 0.0 if ranged else max_dist
        first_ptr = _device_first(s, dev, n, first) if first is not None else None
        if mask is not None:
            m, m_ptr = _mask_args(s, n, mask)
            return _csr_query(s, n, lambda off: spheres_within_masked_count_into(ptr, n, prepared, off, md, md_ptr, first_ptr, m, m_ptr),
                              lambda off, total, idx, gap, row: spheres_within_masked_fill_into(ptr, n, prepared, off, total, idx, gap, row, md,
                                                                                               md_ptr, first_ptr, m, m_ptr),
                              _gap_columns(gaps, rows))
        return _csr_query(s, n, lambda off: spheres_within_count_into(ptr, n, prepared, off, md, md_ptr, first_ptr),
                          lambda off, total, idx, gap, row: spheres_within_fill_into(ptr, n, prepared, off, total, idx, gap, row, md, md_ptr,
                                                                                    first_ptr),
                          _gap_columns(gaps, rows))


def spheres_in_boxes(prepared, boxes, margin=0.0, first=None, gaps=True, rows=False):
    """EVERY sphere that meets every axis-aligned box (rt_spheres_in_boxes_count / _fill), with no cap, in spheres_within's CSR form ->
    (offsets (n + 1,) int64, index (total,) int32, gap (total,) float32 or None[, point (total,) int32]) numpy arrays.  `boxes`: (n, 6)
    float32, rows (lo.xyz, hi.xyz), a numpy array or a device tensor.  Sphere j is selected for box i iff its gap -- in float32,
    e_k = max(lo_k - c_k, c_k - hi_k, 0), gap = sqrtf((ex*ex + ey*ey) + ez*ez) - r: the signed distance from the box to the sphere's surface, -r
    where the centre is inside the box -- is <= the box's margin.  margin 0 is the exact closed sphere / box overlap test (tangency is
    selected).  A box with lo == hi == p selects exactly what spheres_within selects at p with max_dist = margin, with the same gap bits.
    margin: a scalar in [0, 1e9], or an (n,) array / device tensor, one per box (an invalid one gives an empty row).  A box with a
    non-finite component or lo_k > hi_k has an empty row; zero extent is valid.  first, gaps, rows and the row order (ASCENDING sphere index
    into L): as spheres_within."""
    ranged = _is_bound_array(margin)
    with _Scope(prepared.ctx) as s:
        ptr, n = _device_rows(s, boxes, *_BOXES)
        dev = s.ctx.device_info()["device"]
        mg_ptr = _device_bound(s, dev, n, "margin", margin, per="box") if ranged else None
        mg = 0.0 if ranged else margin
        first_ptr = _device_first(s, dev, n, first, per="box") if first is not None else None
        return _csr_query(s, n, lambda off: spheres_in_boxes_count_into(ptr, n, prepared, off, mg, mg_ptr, first_ptr),
                          lambda off, total, idx, gap, row: spheres_in_boxes_fill_into(ptr, n, prepared, off, total, idx, gap, row, mg, mg_ptr,
                                                                                      first_ptr),
                          _gap_columns(gaps, rows))


_PLANES_SHAPE = "planes must be (n, K, 4) with 1 <= K <= 8: rows a, b, c, d"


def _device_planes(scope, planes):
    """(pointer, n, K) for `planes` (n x K x 4 float32): a numpy array is uploaded to a buffer of the scope; a contiguous float32 torch tensor
    on the context's device is used in place."""
    if hasattr(planes, "data_ptr"):
        _check_tensor(planes, scope.ctx.device_info()["device"], "float32", "planes")
        shape = tuple(planes.shape)
        ptr = planes.data_ptr()
    else:
        planes = np.ascontiguousarray(planes, dtype=np.float32)
        shape = planes.shape
        ptr = None
    if len(shape) != 3 or shape[2] != 4 or not 1 <= shape[1] <= 8:
        raise ValueError(_PLANES_SHAPE)
    return (scope.upload(planes) if ptr is None else ptr), int(shape[0]), int(shape[1])


def spheres_in_planes(prepared, planes, margin=0.0, first=None, gaps=True, rows=False):
    """EVERY sphere inside every query's planes -- a frustum, a slab, an oriented box, any convex polytope of up to 8 half-spaces
    (rt_spheres_in_planes_count / _fill) -- with no cap, in spheres_in_boxes's CSR form -> (offsets (n + 1,) int64, index (total,) int32,
    gap (total,) float32 or None[, point (total,) int32]) numpy arrays.  `planes`: (n, K, 4) float32, rows (a, b, c, d) whose inside is
    a x + b y + c z + d >= 0 (normals point inward), a numpy array or a device tensor; a query that needs fewer than K planes repeats one.
    Each plane is normalised in float32 (len = sqrtf((a*a + b*b) + c*c), n = (a, b, c) / len, w = d / len), depth_k = ((nx*cx + ny*cy) +
    nz*cz) + w, and sphere j is selected for query i iff gap = max(0, -depth_0, ..., -depth_{K-1}) - r <= the query's margin.  margin 0 is
    "the closed ball meets every closed half-space", the standard frustum-culling test: conservative for the polytope (a sphere outside an
    edge or a corner can be selected; one that meets the polytope is never dropped).  A centre inside every half-space has gap -r.
    margin: a scalar in [0, 1e9], or an (n,) array / device tensor, one per query (an invalid one gives an empty row).  A query with a
    non-finite plane or a normal whose length is outside [2^-40, 2^40] has an empty row.  first, gaps, rows and the row order (ASCENDING
    sphere index into L): as spheres_within.  frustum_planes and tile_frusta make the planes of a camera."""
    ranged = _is_bound_array(margin)
    with _Scope(prepared.ctx) as s:
        ptr, n, k = _device_planes(s, planes)
        dev = s.ctx.device_info()["device"]
        mg_ptr = _device_bound(s, dev, n, "margin", margin, per="query") if ranged else None
        mg = 0.0 if ranged else margin
        first_ptr = _device_first(s, dev, n, first, per="query") if first is not None else None
        return _csr_query(s, n, lambda off: spheres_in_planes_count_into(ptr, n, k, prepared, off, mg, mg_ptr, first_ptr),
                          lambda off, total, idx, gap, row: spheres_in_planes_fill_into(ptr, n, k, prepared, off, total, idx, gap, row, mg,
                                                                                       mg_ptr, first_ptr),
                          _gap_columns(gaps, rows))


def _unit(v):
    return v / np.sqrt((v * v).sum())


def frustum_planes(cam12, u0=0.0, u1=1.0, v0=0.0, v1=1.0, near=None, far=None):
    """The planes of the part [u0, u1] x [v0, v1] of a camera's image (cam12: origin, lower-left corner, horizontal, vertical, as
    Prepared.camera() and rt_camera_rays; the ray of (u, v) has direction llc + u * horizontal + v * vertical - origin) -> (4 | 5 | 6, 4)
    float32 rows (a, b, c, d) with unit inward normals, computed in float64: left (u = u0), right (u = u1), bottom (v = v0), top (v = v1),
    then the near and the far plane where given.  Each side plane passes through the origin, contains two corner directions and is oriented so
    that the central direction has positive depth.  near / far: distances from the origin along the unit normal of the image plane,
    cross(horizontal, vertical), oriented towards llc - origin."""
    c = np.asarray(cam12, dtype=np.float64).reshape(12)
    o, llc, hor, ver = c[0:3], c[3:6], c[6:9], c[9:12]
    d = lambda u, v: llc + u * hor + v * ver - o   # noqa: E731
    mid = d(0.5 * (u0 + u1), 0.5 * (v0 + v1))
    out = []
    for p, q in ((d(u0, v0), d(u0, v1)), (d(u1, v0), d(u1, v1)), (d(u0, v0), d(u1, v0)), (d(u0, v1), d(u1, v1))):
        n = _unit(np.cross(p, q))
        if n @ mid < 0.0:
            n = -n
        out.append(np.append(n, -(n @ o)))
    f = _unit(np.cross(hor, ver))
    if f @ (llc - o) < 0.0:
        f = -f
    if near is not None:
        out.append(np.append(f, -(f @ o) - float(near)))
    if far is not None:
        out.append(np.append(-f, (f @ o) + float(far)))
    return np.ascontiguousarray(np.stack(out), dtype=np.float32)


def tile_frusta(cam12, h, w, tile_h, tile_w):
    """The side planes of every tile of an h x w frame cut into tiles of tile_h x tile_w pixels (the last row and column of tiles may be
    smaller) -> (tiles_y * tiles_x, 4, 4) float32, tiles row-major from the top row, each frustum_planes of the tile's part of the image:
    the tile of rows [y0, y1) and columns [x0, x1) gets u in [x0 / w, x1 / w] and v in [(h - y1) / h, (h - y0) / h] -- rt_camera_rays puts
    row 0 at v = 1 -- which holds the primary ray of each of its pixels."""
    h, w, tile_h, tile_w = int(h), int(w), int(tile_h), int(tile_w)
    if h < 1 or w < 1 or tile_h < 1 or tile_w < 1:
        raise ValueError("tile_frusta: h, w, tile_h and tile_w must be positive")
    out = []
    for y0 in range(0, h, tile_h):
        y1 = min(h, y0 + tile_h)
        for x0 in range(0, w, tile_w):
            x1 = min(w, x0 + tile_w)
            out.append(frustum_planes(cam12, x0 / w, x1 / w, (h - y1) / h, (h - y0) / h))
    return np.ascontiguousarray(np.stack(out), dtype=np.float32)


def spheres_along_rays(prepared, rays, radius=0.0, t_min=0.0, t_max=1e9, exclude=None, first=None, roots=True, rows=False):
    """EVERY sphere a ray crosses (radius 0) or a moving sphere of radius `radius` touches over (t_min, t_max), with no cap
    (rt_spheres_along_rays_count / _fill), in spheres_within's CSR form -> (offsets (n + 1,) int64, index (total,) int32, roots (total, 2)
    float32 or None, start (total,) uint8[, query (total,) int32]) numpy arrays.  The selection is sweep_spheres's: row i holds every contact
    sweep_spheres would count for query i -- its length is that count -- in ASCENDING sphere index (an index into L), not by time.  roots:
    the two roots t1 <= t2 of the ray against the sphere widened by the query's radius, unclamped (t1 may lie before t_min, t2 past t_max);
    start: 0 for an entry contact (the contact is at t1), 1 for an overlap that already exists where the interval begins (the contact is at
    t_min).  row_contacts turns rows into sweep_spheres's view (by time, padded to k), row_crossings into multi_hit_rays's.
    radius, t_min, t_max: each a scalar, or an (n,) array / float32 device tensor, one per query (a scalar next to an array bound is
    broadcast; an invalid array value gives an empty row; an invalid scalar, or a scalar pair with t_min > t_max, is an RtError).  exclude:
    None, or an (n,) integer array / int32 device tensor -- sphere exclude[i] is skipped for query i.  first: as spheres_within.
    roots=False: no roots array (None in its place).  rows=True: also `query`, the row number of every entry.  `rays`: (n, 6) float32, a
    numpy array or a device tensor."""
    with _Scope(prepared.ctx) as s:
        ptr, n = _device_rows(s, rays, *_RAYS)
        dev = s.ctx.device_info()["device"]
        kw = {"radius": 0.0, "t_min": 0.0, "t_max": 0.0}
        if _is_bound_array(radius):
            kw["radius_ptr"] = _device_bound(s, dev, n, "radius", radius, per="query")
        else:
            kw["radius"] = radius
        if _is_bound_array(t_min) or _is_bound_array(t_max):
            kw["t_min_ptr"] = _device_bound(s, dev, n, "t_min", t_min, per="query")
            kw["t_max_ptr"] = _device_bound(s, dev, n, "t_max", t_max, per="query")
        else:
            if not np.float32(t_min) <= np.float32(t_max):
                raise RtError(f"t_min = {t_min!r}, t_max = {t_max!r}: scalar bounds must satisfy t_min <= t_max")
            kw["t_min"], kw["t_max"] = t_min, t_max
        kw["exclude_ptr"] = _device_first(s, dev, n, exclude, name="exclude", per="query") if exclude is not None else None
        kw["first_ptr"] = _device_first(s, dev, n, first, per="query") if first is not None else None
        return _csr_query(s, n, lambda off: spheres_along_rays_count_into(ptr, n, prepared, off, **kw),
                          lambda off, total, idx, rts, st, row: spheres_along_rays_fill_into(ptr, n, prepared, off, total, idx, rts, st, row, **kw),
                          ((np.int32, 1, True), (np.float32, 2, bool(roots)), (np.uint8, 1, True), (np.int32, 1, True if rows else None)))


def _row_bound(n, b):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(b, dtype=np.float32), (n,)))


def _ranked_rows(n, k, row, keys, columns):
    """Entries with row numbers `row` sorted by (row, keys...), the first k of every row scattered into (n, k) arrays: `columns` is a list of
    (values, padding, dtype) -> (count (n,) int32, [array (n, k) ...])."""
    k = int(k)
    order = np.lexsort(tuple(reversed(keys)) + (row,))
    row = row[order]
    count = np.bincount(row, minlength=n).astype(np.int32)
    begin = np.concatenate([[0], np.cumsum(count, dtype=np.int64)[:-1]])
    slot = np.arange(row.size) - begin[row]
    sel = slot < k
    out = []
    for values, pad, dtype in columns:
        a = np.full((n, k), pad, dtype)
        a[row[sel], slot[sel]] = values[order][sel]
        out.append(a)
    return count, out


def row_contacts(offsets, index, roots, start, t_min, k):
    """The rows of spheres_along_rays as sweep_spheres sees them -> (count (n,) int32, index (n, k) int32, start (n, k) uint8, tau (n, k)
    float32): every row ordered by (tau, index) with tau = t_min + 0.0 for an overlap at the start and t1 for an entry contact, the first
    min(count, k) kept, the slots past them -1, 0 and 0.0 -- sweep_spheres's count, index, start and hit[..., 0] for the same queries.
    t_min: the queries' scalar t_min, or their (n,) array.  Host-side numpy on the arrays spheres_along_rays returned."""
    offsets = np.asarray(offsets, dtype=np.int64)
    n = offsets.size - 1
    row = np.repeat(np.arange(n), np.diff(offsets))
    index, start = np.asarray(index), np.asarray(start)
    lo = _row_bound(n, t_min)
    with np.errstate(invalid="ignore"):
        tau = np.where(start != 0, lo[row] + np.float32(0), np.asarray(roots, dtype=np.float32).reshape(-1, 2)[:, 0]).astype(np.float32)
    count, (idx, st, tk) = _ranked_rows(n, k, row, (tau, index), ((index, -1, np.int32), (start, 0, np.uint8), (tau, 0, np.float32)))
    return count, idx, st, tk


def row_crossings(offsets, index, roots, t_min, t_max, k):
    """The rows of spheres_along_rays (radius 0) as multi_hit_rays sees them -> (count (n,) int32, index (n, k) int32, root (n, k) uint8,
    t (n, k) float32): the roots of every row's entries that lie strictly inside (t_min, t_max), ordered by (t, index, root) with root 1
    for t1 and 2 for t2, the first min(count, k) kept, the slots past them -1, 0 and 0.0 -- multi_hit_rays's count, index, root and
    hit[..., 0] for the same rays.  An entry with no root inside the interval (the segment lies wholly inside the sphere) contributes none.
    t_min, t_max: the queries' scalars, or their (n,) arrays.  Host-side numpy on the arrays spheres_along_rays returned."""
    offsets = np.asarray(offsets, dtype=np.int64)
    n = offsets.size - 1
    row = np.repeat(np.arange(n), np.diff(offsets))
    index = np.asarray(index)
    roots = np.asarray(roots, dtype=np.float32).reshape(-1, 2)
    lo, hi = _row_bound(n, t_min)[row], _row_bound(n, t_max)[row]
    t = np.concatenate([roots[:, 0], roots[:, 1]])
    with np.errstate(invalid="ignore"):
        keep = (t > np.concatenate([lo, lo])) & (t < np.concatenate([hi, hi]))
    which = np.concatenate([np.full(row.size, 1, np.uint8), np.full(row.size, 2, np.uint8)])[keep]
    row2, idx2, t = np.concatenate([row, row])[keep], np.concatenate([index, index])[keep], t[keep]
    count, (idx, rt, tk) = _ranked_rows(n, k, row2, (t, idx2, which), ((idx2, -1, np.int32), (which, 0, np.uint8), (t, 0, np.float32)))
    return count, idx, rt, tk


def visible_pairs(prepared, points, targets=None, directions=None, t_min=0.0, t_max=1e9, mask=True, count=True, words_per_wave=0):
    """The visibility matrix of every point against every target or direction (rt_visible_pairs) -> (visible (n, W) uint64 or None, count
    (n,) int32 or None) numpy arrays, W = (m + 63) // 64.  Exactly one of `targets` (m positions: the ray of pair (i, j) is o = points[i],
    d = targets[j] - points[i] in float32; a shadow test is t_min = eps, t_max = 1) and `directions` (m directions: d = directions[j];
    ambient occlusion is t_min = eps, t_max = the radius) is given.  Bit j & 63 of visible[i, j >> 6] is 1 iff the pair is valid -- o and d
    finite, d not zero -- and occluded_rays answers False for its ray over (t_min, t_max); the bits past m are 0; count[i] is the number of
    set bits of row i.  unpack_visible(visible, m) is the (n, m) bool matrix.  No n x m ray buffer is made: the rays exist in registers
    only.  mask=False / count=False: that output is not computed (None in its place; not both).  `points`, `targets`, `directions`:
    (., 3) float32, numpy arrays or device tensors used in place.  words_per_wave: as visible_pairs_into."""
    if (targets is None) == (directions is None):
        raise ValueError("visible_pairs: exactly one of targets and directions must be given")
    if not mask and not count:
        raise ValueError("visible_pairs: mask and count cannot both be False")
    mode = PAIRS_TARGETS if directions is None else PAIRS_DIRECTIONS
    with _Scope(prepared.ctx) as s:
        ptr, n = _device_rows(s, points, *_POINTS)
        tptr, m = (_device_rows(s, targets, "targets", 3, "targets must be (m, 3)") if directions is None else
                   _device_rows(s, directions, "directions", 3, "directions must be (m, 3)"))
        words = (m + 63) // 64
        vis = s.alloc(8 * n * words) if mask else None
        cnt = s.alloc(4 * n) if count else None
        visible_pairs_into(ptr, n, tptr, m, prepared, mode, vis.ptr if vis else None, cnt.ptr if cnt else None, t_min, t_max, words_per_wave)
        return (vis.to_host((n, words), np.uint64) if vis else None, cnt.to_host((n,)) if cnt else None)


def unpack_visible(words, m):
    """The (n, m) bool matrix of visible_pairs's (n, W) uint64 words (little-endian: bit j & 63 of word j >> 6 is pair j).  Host-side numpy."""
    w = np.ascontiguousarray(words, dtype="<u8")
    if w.ndim != 2 or not 0 <= int(m) <= 64 * w.shape[1]:
        raise ValueError("unpack_visible: words must be (n, W) with m <= 64 * W")
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[0], 8 * w.shape[1]), axis=1, bitorder="little")
    return bits[:, :int(m)].astype(bool)


def contact_pairs(prepared, margin=0.0, gaps=True):
    """The scene's contact pairs (rt_contact_pairs_count / _fill), with no cap -> (pairs (m, 2) int32, gap (m,) float32 or None) numpy arrays.
    Pair (i, j), i < j, is reported once iff gap(centre_i, L[j]) = sqrtf(|c_i - c_j|^2) - r_j <= r_i + margin, all in float32 and evaluated
    from the lower index only; rows in ascending (i, j).  `gap` is that gap (subtract r_i for the surface-to-surface distance).  i and j are
    indices into L (Morton order): prepared.sphere_ids() maps them to the caller's order.  margin: a scalar in [0, 1e9]."""
    n = prepared.num_spheres
    with _Scope(prepared.ctx) as s:
        return _csr_query(s, n, lambda off: contact_pairs_count_into(prepared, off, margin),
                          lambda off, total, pair, gap: contact_pairs_fill_into(prepared, off, total, pair, gap, margin),
                          ((np.int32, 2, True), (np.float32, 1, bool(gaps))))[1:]


def contact_clusters(prepared, margin=0.0):
    """The connected components of the scene's contact graph (rt_contact_clusters) -> (root (n,) int32, cluster (n,) int32, size (n,) int32,
    num int) with numpy arrays.  The edges are exactly contact_pairs(prepared, margin)'s rows; no pair list is built.  root[i] is the
    smallest index in i's component (root[i] == i marks one representative per cluster), cluster[i] a dense id in [0, num) numbered in
    ascending order of the root, size[i] the number of spheres in i's cluster.  All indices are into L (Morton order):
    prepared.sphere_ids() maps them to the caller's order.  margin: a scalar in [0, 1e9]."""
    n = prepared.num_spheres
    with _Scope(prepared.ctx) as s:
        root, cluster, size, num = s.alloc(4 * n), s.alloc(4 * n), s.alloc(4 * n), s.alloc(8)
        contact_clusters_into(prepared, root.ptr, cluster.ptr, size.ptr, num.ptr, margin)
        return root.to_host((n,)), cluster.to_host((n,)), size.to_host((n,)), int(num.to_host((1,), np.int64)[0])


def cluster_members(cluster, num):
    """The member list of each cluster in CSR form -> (offsets (num + 1,) int64, members (n,) int32): cluster c holds
    members[offsets[c]:offsets[c + 1]], ascending.  `cluster` and `num` as contact_clusters returns them; the members are indices into L
    (prepared.sphere_ids() maps them to the caller's order).  Host-side numpy: a stable argsort."""
    c = np.ascontiguousarray(cluster)
    num = int(num)
    if c.ndim != 1 or c.dtype.kind not in "iu" or num < 0 or (c.size and (int(c.min()) < 0 or int(c.max()) >= num)):
        raise ValueError("cluster_members: cluster must be a 1-d integer array with values in [0, num)")
    offsets = np.zeros(num + 1, np.int64)
    np.cumsum(np.bincount(c, minlength=num), out=offsets[1:])
    return offsets, np.argsort(c, kind="stable").astype(np.int32)


def camera_rays(prepared, h, w, cam=None):
    """The primary rays of an h x w frame (rt_camera_rays) -> (h * w, 6) float32 numpy array, row-major from the top row."""
    ctx = prepared.ctx
    buf = DeviceBuffer(ctx, 24 * int(h) * int(w))
    try:
        camera_rays_into(buf.ptr, h, w, prepared, cam)
        return buf.to_host((int(h) * int(w), 6), np.float32)
    finally:
        buf.free()
