"""Python mirror of OpenCorr's hot-path classes over the HIP C-ABI.

Same names, constructor arguments and call order as the reference
(``src/oc_fftcc.h:54-89``, ``src/oc_icgn.h:45-180``, ``src/oc_dic.h:43-84``):

    fftcc = FFTCC2D(rx, ry);            fftcc.set_images(ref, tar); fftcc.compute(pois)
    icgn  = ICGN2D1(rx, ry, conv, stop); icgn.set_images(ref, tar);  icgn.prepare(); icgn.compute(pois)

``pois`` is the reference's POI2D/POI3D AoS as a float32 array of shape (n, 25) /
(n, 31), updated in place: a NumPy array takes the host path (H2D, kernels,
D2H), a CUDA torch tensor is used in place on the device.  Images are NumPy
arrays (uploaded) or CUDA torch tensors (row-major, used in place).
"""
import ctypes

import numpy as np

from . import capi


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _buf(x, floats_per_row=None):
    """(pointer, memory kind, keep-alive) of a float32 NumPy array or CUDA torch tensor."""
    if _is_torch(x):
        import torch
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("torch buffers must be contiguous float32")
        if not x.is_cuda:
            raise ValueError("torch buffers must live on the GPU (pass NumPy arrays for host data)")
        return ctypes.c_void_p(x.data_ptr()), capi.DEVICE, x
    a = np.ascontiguousarray(x, dtype=np.float32)
    return ctypes.c_void_p(a.ctypes.data), capi.HOST, a


class _Engine:
    _ndim = 2

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        self._keep = []
        self._device = int(device)   # where the engine lives (set_devices()[0] moves it)
        self._stream_pinned = False  # set_stream() was called by the user
        self._auto_stream = None     # torch stream adopted for CUDA-tensor arguments
        self._on_private_stream = True  # False once any caller-owned stream (pinned or adopted) is in use

    # -- lifecycle ---------------------------------------------------------
    def close(self):
        if self._h:
            capi.lib().oc_hip_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- DIC::setImages / DVC::setImages ------------------------------------
    def set_images(self, ref, tar, layout=capi.ROW_MAJOR):
        """``layout=COL_MAJOR``: the arrays have the logical shape (height, width) but Fortran
        (Eigen::MatrixXf) memory order; NumPy inputs are converted with ``np.asfortranarray``."""
        if layout == capi.COL_MAJOR and not _is_torch(ref):
            ref = np.asfortranarray(ref, dtype=np.float32)
            tar = np.asfortranarray(tar, dtype=np.float32)
            rp, rmem, rkeep = ctypes.c_void_p(ref.ctypes.data), capi.HOST, ref
            tp, tmem, tkeep = ctypes.c_void_p(tar.ctypes.data), capi.HOST, tar
        else:
            self._adopt_stream_of(ref)
            rp, rmem, rkeep = _buf(ref)
            tp, tmem, tkeep = _buf(tar)
        if rmem != tmem:
            raise ValueError("reference and target image must live in the same memory space")
        shape = tuple(rkeep.shape)
        if tuple(tkeep.shape) != shape or len(shape) != self._ndim:
            raise ValueError("bad image shapes %r / %r" % (shape, tuple(tkeep.shape)))
        if self._ndim == 2:
            h, w = shape
            capi.check(capi.lib().oc_hip_set_images2d(self._h, rp, tp, h, w, layout, rmem))
        else:
            dz, dy, dx = shape
            capi.check(capi.lib().oc_hip_set_images3d(self._h, rp, tp, dx, dy, dz, rmem))
        # device images are used in place: keep them alive
        self._keep = [rkeep, tkeep] if rmem == capi.DEVICE else []
        self.shape = shape

    def share_images(self, donor):
        """Use the donor's device-resident image pair (one upload for an FFTCC + ICGN pair).  The borrower also joins the
        stream the donor runs on (pinned with ``set_stream`` or adopted from a CUDA tensor), unless it was given a
        stream of its own: the donor's images may still be in flight on that stream, and ``prepare()`` receives no tensor
        it could take the stream from -- on its private stream it would read them too early."""
        capi.check(capi.lib().oc_hip_share_images(self._h, donor._h))
        # the pair is the borrower's from here on (the engine holds its own reference): device images used in place must
        # outlive the donor's next set_images too
        self._keep = [donor] + list(donor._keep)
        self.shape = donor.shape
        if not self._stream_pinned and not getattr(donor, "_on_private_stream", True):
            s = donor._auto_stream
            capi.check(capi.lib().oc_hip_set_stream(self._h, ctypes.c_void_p(s or None)))
            self._auto_stream = s
            self._on_private_stream = False

    def set_subset(self, rx, ry, rz=0):
        capi.check(capi.lib().oc_hip_set_subset(self._h, rx, ry, rz))

    def set_stream(self, stream_handle):
        """Run on a caller-owned hipStream_t (0 / None = HIP's default stream, as torch reports it)."""
        capi.check(capi.lib().oc_hip_set_stream(self._h, ctypes.c_void_p(stream_handle or None)))
        self._stream_pinned = True
        self._auto_stream = stream_handle or None
        self._on_private_stream = False

    def _adopt_stream_of(self, x):
        """CUDA torch tensors are produced on torch's current stream: unless the user pinned a stream, the engine
        runs on that stream too, so the tensor is read after whatever wrote it and torch ops that follow see the
        results (stream order instead of timing).  From then on the engine STAYS on that stream (until
        ``reset_stream``): DEVICE-queue computes are asynchronous, and later NumPy / host-queue calls run on it too.
        A tensor that lives on another GPU than the engine is refused (its stream belongs to that device)."""
        if not _is_torch(x) or not x.is_cuda:
            return
        dev = getattr(self, "_device", None)
        if dev is not None and x.device.index is not None and x.device.index != dev:
            raise ValueError("tensor lives on cuda:%d but the engine on device %d" % (x.device.index, dev))
        if self._stream_pinned:
            return
        import torch
        s = torch.cuda.current_stream(x.device).cuda_stream or None
        if getattr(self, "_on_private_stream", True) or s != self._auto_stream:
            capi.check(capi.lib().oc_hip_set_stream(self._h, ctypes.c_void_p(s)))
            self._auto_stream = s
            self._on_private_stream = False

    def set_devices(self, device_ids):
        """Spread this engine over several GPUs of the node (``oc_hip_set_devices``): contiguous blocks of every
        queue, one per device; setters, images, prepare() and compute() fan out.  ``device_ids[0]`` is the engine's
        own device (it moves there if needed -- set the images again).  Results do not depend on the group size."""
        ids = (ctypes.c_int * len(device_ids))(*[int(d) for d in device_ids])
        capi.check(capi.lib().oc_hip_set_devices(self._h, ids, len(device_ids)))
        if int(device_ids[0]) != self._device:
            # the engine moved: it is back on a fresh private stream of the new device
            self._device = int(device_ids[0])
            self._stream_pinned = False
            self._auto_stream = None
            self._on_private_stream = True

    def devices(self):
        n = ctypes.c_int()
        capi.check(capi.lib().oc_hip_get_devices(self._h, None, 0, ctypes.byref(n)))
        ids = (ctypes.c_int * n.value)()
        capi.check(capi.lib().oc_hip_get_devices(self._h, ids, n.value, ctypes.byref(n)))
        return list(ids)

    def group_queue(self, member):
        """(device pointer, bytes per block) of a member's all-gathered copy of the last DEVICE queue."""
        ptr = ctypes.c_void_p()
        blk = ctypes.c_size_t()
        capi.check(capi.lib().oc_hip_group_queue(self._h, int(member), ctypes.byref(ptr), ctypes.byref(blk)))
        return ptr.value, blk.value

    def set_tuning(self, key, value):
        """Knob of the C-ABI (``oc_hip_set_tuning``).  Every key but two selects among kernels that compute the same bits;
        ``"arith_fma"`` = 1 switches the ICGN / IC-LM solvers to the fused arithmetic contract (one rounding fewer per
        per-sample multiply-add: oracle order ``ORDER_LANES_FMA``; results move by rounding, inside the 1e-4 tolerance).
        ``"arith_onepass"`` = 1 (ICGN2D1 / ICGN2D2 only) selects the one-pass arithmetic contract: an iteration is one sweep with
        3 + DOF running sums and no target array; bit-exact against ``tests/cpp/icgn2d_onepass_twin.cpp``, same distance bars
        against the reference's order; ``arith_fma`` does not matter under it.  ``compute_with_offsets`` and
        ``set_self_adaptive(True)`` raise under it, and the set-up cache is not used.
        ``"arith_onepass3d"`` = 1 (ICGN3D1 only) is the same contract for DVC: the tap sweep forms 15 running sums, no warped
        sample is stored and no scratch is reserved; bit-exact against ``tests/cpp/icgn3d_onepass_twin.cpp``; ``arith_fma`` does
        not matter under it.  ICGN3D1 refuses ``"arith_onepass"`` and names this key."""
        capi.check(capi.lib().oc_hip_set_tuning(self._h, key.encode(), int(value)))

    def reset_stream(self):
        capi.check(capi.lib().oc_hip_reset_stream(self._h))
        self._stream_pinned = False
        self._auto_stream = None
        self._on_private_stream = True

    def prepare(self):
        capi.check(capi.lib().oc_hip_prepare(self._h))

    def prepare_ref(self):
        capi.check(capi.lib().oc_hip_prepare_ref(self._h))

    def prepare_tar(self):
        capi.check(capi.lib().oc_hip_prepare_tar(self._h))

    # -- compute(std::vector<POI>&) -------------------------------------------
    def compute(self, pois):
        floats = capi.POI2D_FLOATS if self._ndim == 2 else capi.POI3D_FLOATS
        self._adopt_stream_of(pois)
        if _is_torch(pois):
            p, mem, _ = _buf(pois)
            n, stride = pois.shape[0], pois.stride(0) * 4
            if pois.shape[1] < floats:
                raise ValueError("POI records need %d floats" % floats)
        else:
            if pois.dtype != np.float32 or not pois.flags.c_contiguous or pois.ndim != 2 or pois.shape[1] < floats:
                raise ValueError("pois must be a C-contiguous float32 array of shape (n, >=%d)" % floats)
            p, mem = ctypes.c_void_p(pois.ctypes.data), capi.HOST
            n, stride = pois.shape[0], pois.strides[0]
        capi.check(capi.lib().oc_hip_compute(self._h, p, n, stride, mem))
        return pois

    def compute_with_offsets(self, pois, center_offsets):
        """compute(poi_queue, center_offset_queue) of ICGN2D1/2D2 (src/oc_icgn.h:76,131);
        ``center_offsets`` is (n, 2) float32 (Point2D x, y) in the same memory space as ``pois``."""
        floats = capi.POI2D_FLOATS
        self._adopt_stream_of(pois)
        if _is_torch(pois):
            p, mem, _ = _buf(pois)
            o, omem, _ = _buf(center_offsets)
            if omem != mem:
                raise ValueError("POIs and center offsets must live in the same memory space")
            n, stride = pois.shape[0], pois.stride(0) * 4
        else:
            if pois.dtype != np.float32 or not pois.flags.c_contiguous or pois.ndim != 2 or pois.shape[1] < floats:
                raise ValueError("pois must be a C-contiguous float32 array of shape (n, >=%d)" % floats)
            off = np.ascontiguousarray(center_offsets, dtype=np.float32)
            p, mem = ctypes.c_void_p(pois.ctypes.data), capi.HOST
            o = ctypes.c_void_p(off.ctypes.data)
            n, stride = pois.shape[0], pois.strides[0]
        if tuple(center_offsets.shape) != (n, 2):
            raise ValueError("center_offsets must have shape (n, 2)")
        capi.check(capi.lib().oc_hip_compute_with_offsets(self._h, p, o, n, stride, mem))
        return pois

    def select_best(self, candidates, segment_starts, pois):
        """Keeps, for POI s, the candidate with the highest ZNCC among candidates[segment_starts[s]:segment_starts[s+1]]
        (deformation and result vectors are copied into pois[s]) -- the selection step of
        EpipolarSearch::compute (src/oc_epipolar_search.cpp:181-190) for a batched candidate queue."""
        self._adopt_stream_of(pois)
        if _is_torch(pois):
            import torch
            cp, mem, _ = _buf(candidates)
            pp_, pmem, _ = _buf(pois)
            if segment_starts.dtype != torch.int32 or not segment_starts.is_cuda or mem != pmem:
                raise ValueError("device queues need an int32 CUDA tensor of segment starts")
            sp = ctypes.c_void_p(segment_starts.data_ptr())
            nc, cs, ns, ps = candidates.shape[0], candidates.stride(0) * 4, pois.shape[0], pois.stride(0) * 4
        else:
            seg = np.ascontiguousarray(segment_starts, dtype=np.uint32)
            self._keep_seg = seg
            cp, mem = ctypes.c_void_p(candidates.ctypes.data), capi.HOST
            pp_ = ctypes.c_void_p(pois.ctypes.data)
            sp = ctypes.c_void_p(seg.ctypes.data)
            nc, cs, ns, ps = candidates.shape[0], candidates.strides[0], pois.shape[0], pois.strides[0]
        if len(segment_starts) != ns + 1:
            raise ValueError("segment_starts needs len(pois) + 1 entries")
        capi.check(capi.lib().oc_hip_select_best(self._h, cp, nc, cs, sp, ns, pp_, ps, mem))
        return pois

    # -- the two selections of the RegionFit -> re-ICGN loop, on the device --------------------------------------
    def _record_floats(self):
        return capi.POI2D_FLOATS if self._ndim == 2 else capi.POI3D_FLOATS

    def _queue_buf(self, x, name, want_mem=None, rows=None, stride_bytes=None):
        """(pointer, memory kind, row stride in bytes) of a POI queue argument, checked the way compute() checks its
        queue: float32, C-contiguous rows of at least one record (the record type is the ENGINE's: a 2D queue padded to
        32 floats per row is still a POI2D queue), CUDA tensor or NumPy array, and -- when other queues of the call are
        already known -- the same memory kind and row stride."""
        floats = self._record_floats()
        if _is_torch(x):
            p, mem, _ = _buf(x)  # float32, contiguous, on the GPU -- or ValueError
            ndim, width, n = x.dim(), x.shape[1] if x.dim() == 2 else 0, x.shape[0]
        else:
            if not isinstance(x, np.ndarray) or x.dtype != np.float32 or not x.flags.c_contiguous:
                raise ValueError("%s must be a C-contiguous float32 NumPy array or a contiguous float32 CUDA tensor" % name)
            p, mem = ctypes.c_void_p(x.ctypes.data), capi.HOST
            ndim, width, n = x.ndim, x.shape[1] if x.ndim == 2 else 0, x.shape[0]
        if ndim != 2 or width < floats:
            raise ValueError("%s must have shape (n, >= %d): POI%dD records" % (name, floats, self._ndim))
        stride = width * 4  # contiguous rows (checked above); an EMPTY array reports a stride of 0, its width does not
        if want_mem is not None and mem != want_mem:
            raise ValueError("%s must live in the same memory space as the POI queue" % name)
        if stride_bytes is not None and stride != stride_bytes:
            raise ValueError("%s must have the POI queue's row stride (%d bytes, got %d)" % (name, stride_bytes, stride))
        if rows is not None and n < rows:
            raise ValueError("%s needs room for %d records (has %d)" % (name, rows, n))
        return p, mem, stride

    @staticmethod
    def _index_buf(index, name, want_mem, rows):
        """pointer of a queue-index list: one 32-bit integer per record, same memory kind as the queues"""
        if _is_torch(index):
            import torch
            # (torch.uint32 exists from torch 2.3 on)
            ok_dtypes = tuple(d for d in (torch.int32, getattr(torch, "uint32", None)) if d is not None)
            if index.dtype not in ok_dtypes or not index.is_contiguous() or index.dim() != 1 or not index.is_cuda:
                raise ValueError("%s must be a contiguous 1-d int32 CUDA tensor" % name)
            mem, n, p = capi.DEVICE, index.shape[0], ctypes.c_void_p(index.data_ptr())
        else:
            if not isinstance(index, np.ndarray) or index.dtype not in (np.uint32, np.int32) or index.ndim != 1 or not index.flags.c_contiguous:
                raise ValueError("%s must be a contiguous 1-d uint32 / int32 NumPy array" % name)
            mem, n, p = capi.HOST, index.shape[0], ctypes.c_void_p(index.ctypes.data)
        if mem != want_mem:
            raise ValueError("%s must live in the same memory space as the POI queue" % name)
        if n < rows:
            raise ValueError("%s needs room for %d entries (has %d)" % (name, rows, n))
        return p

    def split_reliable(self, pois, zncc_threshold_low, zncc_threshold_high, conv_criterion, reliable=None, reliable_offset=0):
        """``oc_hip_split_reliable``: order-preserving partition of a finished queue (examples/
        test_3d_reconstruction_sift_icgn2_regfit.cpp:216-229).  Returns ``(reliable, n_reliable, unreliable, index,
        n_unreliable)``: ``reliable[reliable_offset : reliable_offset + n_reliable]`` and ``unreliable[:n_unreliable]`` hold
        the records, ``index[:n_unreliable]`` the queue positions of the unreliable ones.  CUDA tensors stay on the device
        (the buffers are allocated with ``len(pois)`` records unless ``reliable`` is passed in).  The record type is the
        engine's (POI2D for 2D engines, POI3D for 3D ones), whatever the row width."""
        self._adopt_stream_of(pois)
        reliable_offset = int(reliable_offset)
        if reliable_offset < 0:
            raise ValueError("reliable_offset must not be negative")
        p, mem, stride = self._queue_buf(pois, "pois")
        n, width = pois.shape
        if _is_torch(pois):
            import torch
            if reliable is None:
                reliable = torch.empty((reliable_offset + n, width), dtype=torch.float32, device=pois.device)
            unreliable = torch.empty((n, width), dtype=torch.float32, device=pois.device)
            index = torch.empty((n,), dtype=torch.int32, device=pois.device)
            if not _is_torch(reliable) or reliable.device != pois.device:
                raise ValueError("reliable must be a CUDA tensor on the POI queue's device")
        else:
            if reliable is None:
                reliable = np.zeros((reliable_offset + n, width), dtype=np.float32)
            unreliable = np.zeros((n, width), dtype=np.float32)
            index = np.zeros((n,), dtype=np.uint32)
        rp, _, _ = self._queue_buf(reliable, "reliable", mem, reliable_offset + n, stride)
        up, _, _ = self._queue_buf(unreliable, "unreliable", mem, n, stride)
        ip = self._index_buf(index, "index", mem, n)
        n_rel, n_unr = ctypes.c_size_t(), ctypes.c_size_t()
        capi.check(capi.lib().oc_hip_split_reliable(self._h, p, n, stride, self._ndim, zncc_threshold_low, zncc_threshold_high, conv_criterion,
                                                    rp, reliable_offset, up, ip, ctypes.byref(n_rel), ctypes.byref(n_unr), mem))
        return reliable, n_rel.value, unreliable, index, n_unr.value

    def merge_recovered(self, pois, unreliable, index, n_unreliable, zncc_threshold_high, conv_criterion, reliable, reliable_offset):
        """``oc_hip_merge_recovered``: after RegionFit + ICGN over ``unreliable[:n_unreliable]`` -- the POIs that now pass go
        back into ``pois`` (at their ``index``) and to ``reliable[reliable_offset:]``, the rest move to the front of
        ``unreliable`` / ``index``.  Returns ``(n_recovered, n_remaining)``.  All four buffers must share one memory kind
        (all NumPy or all CUDA tensors on one device), dtype and row stride; an ``index`` entry outside ``pois`` is refused
        (``OC_HIP_ERR_INVALID``) instead of written through."""
        self._adopt_stream_of(pois)
        n_unreliable, reliable_offset = int(n_unreliable), int(reliable_offset)
        if n_unreliable < 0 or reliable_offset < 0:
            raise ValueError("n_unreliable and reliable_offset must not be negative")
        pp_, mem, stride = self._queue_buf(pois, "pois")
        up, _, _ = self._queue_buf(unreliable, "unreliable", mem, n_unreliable, stride)
        rp, _, _ = self._queue_buf(reliable, "reliable", mem, reliable_offset + n_unreliable, stride)
        ip = self._index_buf(index, "index", mem, n_unreliable)
        if mem == capi.DEVICE and not (pois.device == unreliable.device == reliable.device == index.device):
            raise ValueError("pois, unreliable, index and reliable must live on one device")
        n_rec, n_rem = ctypes.c_size_t(), ctypes.c_size_t()
        capi.check(capi.lib().oc_hip_merge_recovered(self._h, pp_, pois.shape[0], stride, self._ndim, up, ip, n_unreliable, zncc_threshold_high,
                                                     conv_criterion, rp, reliable_offset, ctypes.byref(n_rec), ctypes.byref(n_rem), mem))
        return n_rec.value, n_rem.value

    def compute_one(self, poi):
        assert poi.dtype == np.float32 and poi.flags.c_contiguous
        capi.check(capi.lib().oc_hip_compute_one(self._h, ctypes.c_void_p(poi.ctypes.data)))
        return poi

    def synchronize(self):
        capi.check(capi.lib().oc_hip_synchronize(self._h))

    # -- introspection ----------------------------------------------------------
    def read_field(self, name):
        ptr = ctypes.c_void_p()
        count = ctypes.c_size_t()
        capi.check(capi.lib().oc_hip_get_field(self._h, name.encode(), ctypes.byref(ptr), ctypes.byref(count)))
        out = np.empty(count.value, dtype=np.float32)
        capi.check(capi.lib().oc_hip_read_field(self._h, name.encode(), ctypes.c_void_p(out.ctypes.data), count.value))
        if name in ("lut", "lut_gx", "lut_gy"):
            # stored planar [k][y][x][l]; returned in the reference's order coef[y][x][k][l] (src/oc_cubic_bspline.cpp:123-129)
            h, w = self.shape
            return np.ascontiguousarray(out.reshape(4, h, w, 4).transpose(1, 2, 0, 3)).reshape(h, w, 16)
        return out.reshape(self.shape)

    def profile_enable(self, on=True):
        capi.check(capi.lib().oc_hip_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        capi.check(capi.lib().oc_hip_profile_reset(self._h))

    def profile_read(self):
        ms = ctypes.c_double()
        n = ctypes.c_long()
        capi.check(capi.lib().oc_hip_profile_read(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value


class _IcgnMixin:
    def set_iteration(self, conv_criterion, stop_condition):
        capi.check(capi.lib().oc_hip_set_iteration(self._h, conv_criterion, stop_condition))

    def set_self_adaptive(self, is_self_adaptive):
        """DIC::setSelfAdaptive (src/oc_dic.cpp:34-37): per-POI subset radius from poi.subset_radius."""
        capi.check(capi.lib().oc_hip_set_self_adaptive(self._h, 1 if is_self_adaptive else 0))

    def setup_cache_last(self):
        """How the last ICGN2D compute() treated the set-up cache (tuning key "icgn2d_setup_cache"): "none" (went around it),
        "fill" (computed and filed every POI's set-up) or "use" (started from the filed records).  Waits for the engine."""
        state = ctypes.c_int()
        capi.check(capi.lib().oc_hip_icgn2d_setup_cache_last(self._h, ctypes.byref(state)))
        return {capi.SETUP_CACHE_NONE: "none", capi.SETUP_CACHE_FILL: "fill", capi.SETUP_CACHE_USE: "use"}[state.value]


class FFTCC2D(_Engine):
    """FFTCC2D(subset_radius_x, subset_radius_y, thread_number) -- src/oc_fftcc.h:54-68."""

    def __init__(self, subset_radius_x, subset_radius_y, thread_number=1, device=0):
        super().__init__(device)
        self.thread_number = thread_number  # kept for signature compatibility
        capi.check(capi.lib().oc_hip_fftcc2d_create(subset_radius_x, subset_radius_y, device, ctypes.byref(self._h)))


class ICGN2D1(_Engine, _IcgnMixin):
    """ICGN2D1(rx, ry, conv_criterion, stop_condition, thread_number) -- src/oc_icgn.h:45-77."""

    def __init__(self, subset_radius_x, subset_radius_y, conv_criterion, stop_condition, thread_number=1, device=0):
        super().__init__(device)
        self.thread_number = thread_number
        capi.check(capi.lib().oc_hip_icgn2d1_create(subset_radius_x, subset_radius_y, conv_criterion, stop_condition,
                                                    device, ctypes.byref(self._h)))


class ICGN2D2(_Engine, _IcgnMixin):
    """ICGN2D2(rx, ry, conv_criterion, stop_condition, thread_number) -- src/oc_icgn.h:100-132."""

    def __init__(self, subset_radius_x, subset_radius_y, conv_criterion, stop_condition, thread_number=1, device=0):
        super().__init__(device)
        self.thread_number = thread_number
        capi.check(capi.lib().oc_hip_icgn2d2_create(subset_radius_x, subset_radius_y, conv_criterion, stop_condition,
                                                    device, ctypes.byref(self._h)))


class NR2D1(_Engine, _IcgnMixin):
    """NR2D1(rx, ry, conv_criterion, stop_condition, thread_number) -- src/oc_nr.h, src/oc_nr.cpp:75-91."""

    def __init__(self, subset_radius_x, subset_radius_y, conv_criterion, stop_condition, thread_number=1, device=0):
        super().__init__(device)
        self.thread_number = thread_number
        capi.check(capi.lib().oc_hip_nr2d1_create(subset_radius_x, subset_radius_y, conv_criterion, stop_condition,
                                                  device, ctypes.byref(self._h)))


class _IclmMixin(_IcgnMixin):
    def set_damping(self, lambda_, alpha, beta):
        """ICLM2D*::setDamping(lambda, alpha, beta) (src/oc_iclm.cpp:114-119); defaults 100, 0.1, 10."""
        capi.check(capi.lib().oc_hip_set_damping(self._h, lambda_, alpha, beta))


class ICLM2D1(_Engine, _IclmMixin):
    """ICLM2D1(rx, ry, conv_criterion, stop_condition, thread_number) -- src/oc_iclm.h:56-85."""

    def __init__(self, subset_radius_x, subset_radius_y, conv_criterion, stop_condition, thread_number=1, device=0):
        super().__init__(device)
        self.thread_number = thread_number
        capi.check(capi.lib().oc_hip_iclm2d1_create(subset_radius_x, subset_radius_y, conv_criterion, stop_condition,
                                                    device, ctypes.byref(self._h)))


class ICLM2D2(_Engine, _IclmMixin):
    """ICLM2D2(rx, ry, conv_criterion, stop_condition, thread_number) -- src/oc_iclm.h:104-133."""

    def __init__(self, subset_radius_x, subset_radius_y, conv_criterion, stop_condition, thread_number=1, device=0):
        super().__init__(device)
        self.thread_number = thread_number
        capi.check(capi.lib().oc_hip_iclm2d2_create(subset_radius_x, subset_radius_y, conv_criterion, stop_condition,
                                                    device, ctypes.byref(self._h)))


class Strain:
    """Strain(subregion_radius, neighbor_number_min, thread_number) -- src/oc_strain.h:34-73, src/oc_strain.cpp:31-46.

    ``prepare(pois)`` builds the neighbour search over the queue's coordinates, ``compute(pois)`` writes the strain
    fields of every POI that can be fitted, in place (POI2D: exx, eyy, exy; POI3D and POI2DS: exx, eyy, ezz, exy, eyz,
    ezx).  ``pois`` is a float32 (n, 25) / (n, 31) / (n, 28) NumPy array (host path) or CUDA torch tensor (used in place);
    28 floats are the stereo record POI2DS (``P2S``): neighbours over (x, y), the fit over ``ref_coor`` with u, v, w."""

    def __init__(self, subregion_radius, neighbor_number_min, thread_number=1, device=0):
        self._h = ctypes.c_void_p()
        self.thread_number = thread_number
        self._device = int(device)
        self._p = dict(radius=float(subregion_radius), nmin=int(neighbor_number_min), zncc=0.9, approx=1)
        capi.check(capi.lib().oc_hip_strain_create(self._p["radius"], self._p["nmin"], device, ctypes.byref(self._h)))

    def close(self):
        if self._h:
            capi.lib().oc_hip_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _push(self, **kw):
        p = dict(self._p, **kw)
        capi.check(capi.lib().oc_hip_strain_set(self._h, p["radius"], p["nmin"], p["zncc"], p["approx"]))
        self._p = p

    # src/oc_strain.cpp:72-95
    def set_subregion_radius(self, subregion_radius):
        self._push(radius=float(subregion_radius))

    def set_neighbor_min(self, neighbor_number_min):
        self._push(nmin=int(neighbor_number_min))

    def set_zncc_threshold(self, zncc_threshold):
        self._push(zncc=float(zncc_threshold))

    def set_approximation(self, approximation):
        """1 = Cauchy strain, 2 = Green strain."""
        self._push(approx=int(approximation))

    set_stream = _Engine.set_stream
    _adopt_stream_of = _Engine._adopt_stream_of
    _stream_pinned = False
    _auto_stream = None
    _on_private_stream = True

    def synchronize(self):
        capi.check(capi.lib().oc_hip_synchronize(self._h))

    @staticmethod
    def _queue(pois):
        if _is_torch(pois):
            p, mem, _ = _buf(pois)
            n, floats, stride = pois.shape[0], pois.shape[1], pois.stride(0) * 4
        else:
            if pois.dtype != np.float32 or not pois.flags.c_contiguous or pois.ndim != 2:
                raise ValueError("pois must be a C-contiguous float32 array of shape (n, 25) or (n, 31)")
            p, mem = ctypes.c_void_p(pois.ctypes.data), capi.HOST
            n, floats, stride = pois.shape[0], pois.shape[1], pois.strides[0]
        ndim = {capi.POI2D_FLOATS: 2, capi.POI3D_FLOATS: 3, capi.POI2DS_FLOATS: capi.POI2DS}.get(floats)
        if ndim is None:
            raise ValueError("POI records have 25 (POI2D), 31 (POI3D) or 28 (POI2DS) floats, got %d" % floats)
        return p, n, stride, ndim, mem

    def prepare(self, pois):
        self._adopt_stream_of(pois)
        p, n, stride, ndim, mem = self._queue(pois)
        capi.check(capi.lib().oc_hip_strain_prepare(self._h, p, n, stride, ndim, mem))

    def compute(self, pois):
        self._adopt_stream_of(pois)
        p, n, stride, ndim, mem = self._queue(pois)
        capi.check(capi.lib().oc_hip_strain_compute(self._h, p, n, stride, ndim, mem))
        return pois

    def profile_enable(self, on=True):
        capi.check(capi.lib().oc_hip_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        capi.check(capi.lib().oc_hip_profile_reset(self._h))

    def profile_read(self):
        ms = ctypes.c_double()
        n = ctypes.c_long()
        capi.check(capi.lib().oc_hip_profile_read(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value


# float offsets inside a POI2DS record (src/oc_poi.h:53-60, 73-90, 140-183)
P2S = dict(x=0, y=1, u=2, v=3, w=4, r1r2_zncc=5, r1t1_zncc=6, r1t2_zncc=7, r2_x=8, r2_y=9, t1_x=10, t1_y=11, t2_x=12, t2_y=13,
           ref_x=14, ref_y=15, ref_z=16, tar_x=17, tar_y=18, tar_z=19, exx=20, eyy=21, ezz=22, exy=23, eyz=24, ezx=25,
           srx=26, sry=27)


class _Handle:
    """What Calibration and Stereovision share: the handle's life, its stream."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        self._device = int(device)

    def close(self):
        if self._h:
            capi.lib().oc_hip_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    set_stream = _Engine.set_stream
    _adopt_stream_of = _Engine._adopt_stream_of
    _stream_pinned = False
    _auto_stream = None
    _on_private_stream = True

    def synchronize(self):
        capi.check(capi.lib().oc_hip_synchronize(self._h))

    def profile_enable(self, on=True):
        capi.check(capi.lib().oc_hip_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        capi.check(capi.lib().oc_hip_profile_reset(self._h))

    def profile_read(self):
        ms = ctypes.c_double()
        n = ctypes.c_long()
        capi.check(capi.lib().oc_hip_profile_read(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    @staticmethod
    def _rows(x, floats, what):
        """(pointer, rows, stride in bytes, memory, keep-alive) of an (n, >= floats) float32 array / CUDA tensor whose rows
        may be a view into a wider queue (only the last axis has to be contiguous)."""
        if _is_torch(x):
            import torch
            if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] < floats or not x.is_cuda or (x.shape[1] > 1 and x.stride(1) != 1):
                raise ValueError("%s: need a CUDA float32 tensor of shape (n, >= %d) with contiguous rows" % (what, floats))
            return ctypes.c_void_p(x.data_ptr()), x.shape[0], x.stride(0) * 4, capi.DEVICE, x
        if not isinstance(x, np.ndarray) or x.dtype != np.float32 or x.ndim != 2 or x.shape[1] < floats or x.strides[1] != 4:
            raise ValueError("%s: need a float32 array of shape (n, >= %d) with contiguous rows" % (what, floats))
        return ctypes.c_void_p(x.ctypes.data), x.shape[0], x.strides[0], capi.HOST, x


class Calibration(_Handle):
    """Calibration(intrinsics, extrinsics) -- src/oc_calibration.h:47-97.  ``intrinsics``: fx, fy, fs, cx, cy, k1 ... k6,
    p1, p2; ``extrinsics``: tx, ty, tz, rx, ry, rz.  The matrices are host arithmetic (no GPU needed); ``prepare(height,
    width)`` builds the undistortion map on the device."""

    def __init__(self, intrinsics, extrinsics, device=0):
        super().__init__(device)
        self.intrinsics = np.ascontiguousarray(intrinsics, dtype=np.float32).reshape(13)
        self.extrinsics = np.ascontiguousarray(extrinsics, dtype=np.float32).reshape(6)
        self.height = self.width = 0
        capi.check(capi.lib().oc_hip_calibration_create(ctypes.c_void_p(self.intrinsics.ctypes.data),
                                                        ctypes.c_void_p(self.extrinsics.ctypes.data), self._device,
                                                        ctypes.byref(self._h)))

    def _get(self, what, shape):
        out = np.zeros(shape, dtype=np.float32)
        capi.check(capi.lib().oc_hip_calibration_get(self._h, what, ctypes.c_void_p(out.ctypes.data)))
        return out

    @property
    def intrinsic_matrix(self):
        return self._get(capi.CAL_INTRINSIC, (3, 3))

    @property
    def rotation_matrix(self):
        return self._get(capi.CAL_ROTATION, (3, 3))

    @property
    def translation_vector(self):
        return self._get(capi.CAL_TRANSLATION, (3,))

    @property
    def projection_matrix(self):
        return self._get(capi.CAL_PROJECTION, (3, 4))

    def set_undistortion(self, convergence, iteration):
        capi.check(capi.lib().oc_hip_calibration_set_undistortion(self._h, float(convergence), int(iteration)))

    def prepare(self, height, width):
        capi.check(capi.lib().oc_hip_calibration_prepare(self._h, int(height), int(width)))
        self.height, self.width = int(height), int(width)

    def maps(self):
        """(map_x, map_y) as float32 NumPy arrays of shape (height, width)."""
        mx = np.empty((self.height, self.width), dtype=np.float32)
        my = np.empty_like(mx)
        capi.check(capi.lib().oc_hip_calibration_maps(self._h, ctypes.c_void_p(mx.ctypes.data), ctypes.c_void_p(my.ctypes.data), capi.HOST))
        return mx, my

    def undistort(self, points):
        """Undistorted sensor coordinates of (n, 2) points: a new array / tensor of the same kind."""
        self._adopt_stream_of(points)
        out = points.clone() if _is_torch(points) else np.array(points, dtype=np.float32, order="C")
        src = points if _is_torch(points) else out
        p, n, stride, mem, _ = self._rows(src, 2, "undistort")
        q, _, stride_out, _, _ = self._rows(out, 2, "undistort")
        if stride_out != stride:
            raise ValueError("undistort: rows of the points must be contiguous")
        capi.check(capi.lib().oc_hip_calibration_undistort(self._h, p, q, n, stride, mem))
        return out


class Stereovision(_Handle):
    """Stereovision(view1_cam, view2_cam) -- src/oc_stereovision.h.  Both ``Calibration`` objects are kept alive by this one."""

    def __init__(self, view1_cam, view2_cam, thread_number=1):
        super().__init__(view1_cam._device)
        self.view1_cam, self.view2_cam = view1_cam, view2_cam
        self.thread_number = thread_number
        capi.check(capi.lib().oc_hip_stereo_create(view1_cam._h, view2_cam._h, ctypes.byref(self._h)))

    def close(self):
        super().close()  # before the cameras it points to

    @property
    def fundamental_matrix(self):
        F = np.zeros((3, 3), dtype=np.float32)
        capi.check(capi.lib().oc_hip_stereo_fundamental(self._h, ctypes.c_void_p(F.ctypes.data)))
        return F

    def reconstruct(self, view1_points, view2_points):
        """(n, 3) world coordinates of (n, 2) point pairs (rows may be views into a wider queue)."""
        self._adopt_stream_of(view1_points)
        p1, n, s1, mem, _ = self._rows(view1_points, 2, "reconstruct")
        p2, n2, s2, mem2, _ = self._rows(view2_points, 2, "reconstruct")
        if n != n2 or mem != mem2:
            raise ValueError("reconstruct: the two point queues differ in length or memory space")
        if mem == capi.DEVICE:
            import torch
            out = torch.empty((n, 3), dtype=torch.float32, device=view1_points.device)
            po = ctypes.c_void_p(out.data_ptr())
        else:
            out = np.empty((n, 3), dtype=np.float32)
            po = ctypes.c_void_p(out.ctypes.data)
        capi.check(capi.lib().oc_hip_stereo_reconstruct(self._h, p1, s1, p2, s2, po, 12, n, mem))
        return out

    def reconstruct_pois(self, pois):
        """ref_coor, tar_coor and deformation = tar_coor - ref_coor of every POI2DS record, in place."""
        self._adopt_stream_of(pois)
        p, n, stride, mem, _ = self._rows(pois, capi.POI2DS_FLOATS, "reconstruct_pois")
        capi.check(capi.lib().oc_hip_stereo_reconstruct_pois(self._h, p, n, stride, mem))
        return pois


class DescriptorMatcher(_Handle):
    """DescriptorMatcher(dim, ratio) -- the matching stage of SIFT3D (src/oc_sift.cpp:625-674, 1251-1418, 1420-1487) for
    descriptors computed anywhere: rows of ``dim`` float32 (a multiple of 32 in [32, 1024]; SIFT3D 768, OpenCV's SIFT 128).
    Squared distances are the reference's sequential float32 sums, so the results equal its loops bit for bit
    (``set_tuning("arith_fma", 1)``: the sums a ``-mfma`` build of the reference forms).  NumPy descriptors are copied, CUDA
    torch tensors are used in place; results come back as NumPy arrays unless both sides are CUDA tensors."""

    MONODIRECTIONAL, BIDIRECTIONAL = 0, 1

    def __init__(self, dim, ratio=0.85, device=0):
        super().__init__(device)
        self._dim = int(dim)
        self._side = [None, None]
        self._count = [0, 0]
        capi.check(capi.lib().oc_hip_matcher_create(self._dim, float(ratio), int(device), ctypes.byref(self._h)))

    def set_ratio(self, ratio):
        capi.check(capi.lib().oc_hip_matcher_set_ratio(self._h, float(ratio)))

    def set_tuning(self, key, value):
        """``"arith_fma"`` (0 / 1) and ``"match_splits"`` (0 = automatic, 1 ... 64 parts of the candidate range; same bits)."""
        capi.check(capi.lib().oc_hip_set_tuning(self._h, key.encode(), int(value)))

    def set_descriptors(self, side, rows):
        """``side`` 0 = reference, 1 = target keypoints; ``rows``: (count, dim) float32.  A second call replaces the side."""
        if side not in (0, 1):
            raise ValueError("side must be 0 (reference) or 1 (target)")
        if not _is_torch(rows):
            rows = np.ascontiguousarray(rows, dtype=np.float32)
        if len(rows.shape) != 2 or rows.shape[1] != self._dim:
            raise ValueError("descriptors must have shape (count, %d)" % self._dim)
        self._adopt_stream_of(rows)
        ptr, mem, keep = _buf(rows)
        capi.check(capi.lib().oc_hip_matcher_set_descriptors(self._h, side, ptr, rows.shape[0], mem))
        self._side[side] = keep if mem == capi.DEVICE else None   # a device block is used in place: keep it alive
        self._count[side] = int(rows.shape[0])

    def _on_device(self):
        return self._side[0] is not None and self._side[1] is not None

    def _out(self, n, dtype):
        """(array or tensor, pointer) of n entries where the results go"""
        if self._on_device():
            import torch
            t = torch.empty(n, dtype=torch.int32 if dtype == np.int32 else torch.float32, device=self._side[0].device)
            return t, ctypes.c_void_p(t.data_ptr())
        a = np.empty(n, dtype=dtype)
        return a, ctypes.c_void_p(a.ctypes.data)

    def nearest(self, direction=0):
        """SIFT3D::bruteforceMatch: (matched_idx, best_sq, second_sq), one entry per query; direction 0 = ref -> tar,
        1 = tar -> ref.  matched_idx is -1 where the ratio test fails."""
        n = self._count[0 if direction == 0 else 1]
        mem = capi.DEVICE if self._on_device() else capi.HOST
        idx, pi = self._out(n, np.int32)
        best, pb = self._out(n, np.float32)
        second, ps = self._out(n, np.float32)
        capi.check(capi.lib().oc_hip_matcher_nearest(self._h, int(direction), pi, pb, ps, None, mem))
        return idx, best, second

    def match(self, mode=0):
        """mode 0 = SIFT3D::monodirectionalMatch (pairs in descending target index), 1 = SIFT3D::bidirectionalMatch (ascending
        reference index): (ref_idx, tar_idx)."""
        cap = min(self._count)
        mem = capi.DEVICE if self._on_device() else capi.HOST
        ref, pr = self._out(cap, np.int32)
        tar, pt = self._out(cap, np.int32)
        n = ctypes.c_size_t()
        capi.check(capi.lib().oc_hip_matcher_match(self._h, int(mode), pr, pt, cap, ctypes.byref(n), mem))
        return ref[:n.value], tar[:n.value]


class SIFT3DScaleSpace(_Handle):
    """SIFT3DScaleSpace() -- the extraction half of SIFT3D::compute (src/oc_sift.cpp:676-1249): the Gaussian pyramid, the DoG
    pyramid with ``max_abs`` per layer, the extrema candidates in the reference's scan order (``detect``), their orientation
    (``orient``) and the 768-float descriptors of the accepted keypoints (``describe``).  Volumes are (z, y, x) float32; a NumPy
    volume is copied, a CUDA torch tensor is used in place by ``build``.  Both pyramids stay on the device; ``layer`` downloads
    one.  ``set_tuning("arith_fma", 1)``: fused multiply-adds in the blur sums (the later stages have one arithmetic mode)."""

    CANDIDATE = np.dtype([("x", np.int32), ("y", np.int32), ("z", np.int32), ("octave", np.int32), ("layer", np.int32), ("scale", np.float32)])
    LAYER = np.dtype([("dims", np.int32, 3), ("units", np.float32, 3), ("octave", np.int32), ("scale", np.float32), ("sigma", np.float32),
                      ("max_abs", np.float32)])
    KEYPOINT = np.dtype([("coor_layer", np.float32, 3), ("coor_img", np.float32, 3), ("octave", np.int32), ("layer", np.int32), ("scale", np.float32),
                         ("rotation_matrix", np.float32, 9)])
    GAUSSIAN, DOG = 0, 1
    ACCEPTED, REJECT_GRADIENT, REJECT_EIGENVALUES, REJECT_ANGLE = 0, 1, 2, 3
    DESCRIPTOR_LENGTH = 768

    def __init__(self, device=0):
        super().__init__(device)
        self._volume = None
        self._kp_count = 0
        capi.check(capi.lib().oc_hip_sift3d_create(int(device), ctypes.byref(self._h)))

    def set_tuning(self, key, value):
        """``"arith_fma"`` (0 / 1)."""
        capi.check(capi.lib().oc_hip_set_tuning(self._h, key.encode(), int(value)))

    def set_config(self, n_octave_layers=3, min_dimension=8, alpha=0.1, sigma_source=1.15, sigma_base=1.6):
        """The members of Sift3dConfig the scale space reads; the defaults are SIFT3D::SIFT3D()'s (src/oc_sift.cpp:142-159)."""
        capi.check(capi.lib().oc_hip_sift3d_set_config(self._h, int(n_octave_layers), int(min_dimension), float(alpha), float(sigma_source),
                                                       float(sigma_base)))

    def set_physical_unit(self, unit_x, unit_y, unit_z):
        capi.check(capi.lib().oc_hip_sift3d_set_physical_unit(self._h, float(unit_x), float(unit_y), float(unit_z)))

    def set_volume(self, volume):
        """``volume``: (dim_z, dim_y, dim_x) float32, a NumPy array or a CUDA torch tensor."""
        if len(volume.shape) != 3:
            raise ValueError("the volume must have shape (dim_z, dim_y, dim_x)")
        self._adopt_stream_of(volume)
        ptr, mem, keep = _buf(volume)
        dz, dy, dx = (int(v) for v in volume.shape)
        capi.check(capi.lib().oc_hip_sift3d_set_volume(self._h, ptr, dx, dy, dz, mem))
        self._volume = keep if mem == capi.DEVICE else None   # a device volume is used in place: keep it alive

    def build(self):
        """createGaussianPyramid + createDogPyramid (src/oc_sift.cpp:676-793)."""
        capi.check(capi.lib().oc_hip_sift3d_build(self._h))

    def layers(self, pyramid):
        """One ``LAYER`` record per layer of the Gaussian (0) or DoG (1) pyramid; dims and units are (x, y, z)."""
        n, n_oct = ctypes.c_int(), ctypes.c_int()
        capi.check(capi.lib().oc_hip_sift3d_layer_count(self._h, int(pyramid), ctypes.byref(n), ctypes.byref(n_oct)))
        out = np.zeros(n.value, dtype=self.LAYER)
        for i in range(n.value):
            dims, units = (ctypes.c_int * 3)(), (ctypes.c_float * 3)()
            octave, scale, sigma, max_abs = ctypes.c_int(), ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
            capi.check(capi.lib().oc_hip_sift3d_layer_info(self._h, int(pyramid), i, dims, units, ctypes.byref(octave), ctypes.byref(scale),
                                                           ctypes.byref(sigma), ctypes.byref(max_abs)))
            out[i] = (tuple(dims), tuple(units), octave.value, scale.value, sigma.value, max_abs.value)
        return out

    def layer(self, pyramid, index, out=None):
        """The voxels of one layer as a (dim_z, dim_y, dim_x) float32 array; ``out``: a CUDA torch tensor of that shape to fill instead."""
        dims = (ctypes.c_int * 3)()
        capi.check(capi.lib().oc_hip_sift3d_layer_info(self._h, int(pyramid), int(index), dims, None, None, None, None, None))
        shape = (dims[2], dims[1], dims[0])
        if out is None:
            out = np.empty(shape, dtype=np.float32)
        elif tuple(out.shape) != shape:
            raise ValueError("layer: the output must have shape %r" % (shape,))
        if _is_torch(out):
            ptr, mem, _ = _buf(out)
        else:
            if out.dtype != np.float32 or not out.flags.c_contiguous:
                raise ValueError("layer: the output must be a contiguous float32 array")
            ptr, mem = ctypes.c_void_p(out.ctypes.data), capi.HOST
        capi.check(capi.lib().oc_hip_sift3d_get_layer(self._h, int(pyramid), int(index), ptr, mem))
        return out

    def detect(self):
        """detectExtrema (src/oc_sift.cpp:795-847): a ``CANDIDATE`` array in the reference's scan order."""
        n = ctypes.c_size_t()
        rc = capi.lib().oc_hip_sift3d_detect(self._h, None, 0, ctypes.byref(n), capi.HOST)
        if rc != capi.OK and n.value == 0:
            capi.check(rc)
        out = np.empty(n.value, dtype=self.CANDIDATE)
        if n.value:
            capi.check(capi.lib().oc_hip_sift3d_detect(self._h, ctypes.c_void_p(out.ctypes.data), n.value, ctypes.byref(n), capi.HOST))
        return out

    def set_feature_config(self, beta=0.9, gamma=0.4, gradient_threshold=0.0000000001, truncate_threshold=float(np.float32(0.2) * 128 / 768)):
        """The members of Sift3dConfig ``orient`` and ``describe`` read; the defaults are SIFT3D::SIFT3D()'s (src/oc_sift.cpp:147-152)."""
        capi.check(capi.lib().oc_hip_sift3d_set_feature_config(self._h, float(beta), float(gamma), float(gradient_threshold), float(truncate_threshold)))

    @staticmethod
    def _records(x, dtype, what):
        """(pointer, count, memory kind, keep-alive) of a structured NumPy array of ``dtype`` or a CUDA int32 tensor (n, words)"""
        words = dtype.itemsize // 4
        if _is_torch(x):
            import torch
            if x.dtype != torch.int32 or x.dim() != 2 or x.shape[1] != words or not x.is_cuda or not x.is_contiguous():
                raise ValueError("%s: need a contiguous CUDA int32 tensor of shape (n, %d) (the records' 32-bit words)" % (what, words))
            return ctypes.c_void_p(x.data_ptr()), int(x.shape[0]), capi.DEVICE, x
        a = np.ascontiguousarray(x, dtype=dtype)
        if a.ndim != 1:
            raise ValueError("%s: need a one-dimensional array of records" % what)
        return ctypes.c_void_p(a.ctypes.data), len(a), capi.HOST, a

    def orient(self, candidates=None, with_status=False, on_device=False):
        """assignOrientation (src/oc_sift.cpp:849-1049): the accepted keypoints in candidate order.  ``candidates``: None = the candidates
        of the pyramid as built (what ``detect`` returns), which never leave the device; a ``CANDIDATE`` array; or a CUDA int32 tensor (n, 6) of the same records.
        Results are NumPy (a ``KEYPOINT`` array) unless ``on_device`` or a tensor went in: then a CUDA int32 tensor (n, 18) of the
        records' words.  ``with_status``: also ``status`` (one int per candidate: 0 accepted, 1 gradient threshold, 2 eigenvalues,
        3 angle) and ``sums`` (n, 9: d_x d_y d_z, tensor xx xy xz yy yz zz).  The keypoints also stay on the device for
        ``describe()``."""
        L = capi.lib()
        if candidates is None:
            n_cand = ctypes.c_size_t()
            capi.check(L.oc_hip_sift3d_candidate_count(self._h, ctypes.byref(n_cand)))   # (the list stays where it is)
            ptr, count, mem_in, keep = None, n_cand.value, capi.HOST, None
        else:
            ptr, count, mem_in, keep = self._records(candidates, self.CANDIDATE, "orient")
            if mem_in == capi.DEVICE:
                self._adopt_stream_of(candidates)
                on_device = True
        n = ctypes.c_size_t()
        if on_device:
            import torch
            dev = keep.device if keep is not None and _is_torch(keep) else torch.device("cuda", self._device)
            out = torch.empty((count, 18), dtype=torch.int32, device=dev)
            status = torch.empty(count, dtype=torch.int32, device=dev) if with_status else None
            sums = torch.empty((count, 9), dtype=torch.float32, device=dev) if with_status else None
            p = [ctypes.c_void_p(t.data_ptr()) if t is not None and count else None for t in (out, status, sums)]
            mem = capi.DEVICE
        else:
            out = np.zeros(count, dtype=self.KEYPOINT)
            status = np.zeros(count, np.int32) if with_status else None
            sums = np.zeros((count, 9), np.float32) if with_status else None
            p = [ctypes.c_void_p(a.ctypes.data) if a is not None and count else None for a in (out, status, sums)]
            mem = capi.HOST
        capi.check(L.oc_hip_sift3d_orient(self._h, ptr, count, mem_in, p[0], count, ctypes.byref(n), p[1], p[2], mem))
        self._kp_count = n.value
        out = out[:n.value]
        return (out, status, sums) if with_status else out

    def describe(self, keypoints=None, out=None):
        """constructDescriptor (src/oc_sift.cpp:1051-1249): (n, 768) float32.  ``keypoints``: None = the output of the last
        ``orient``, which is on the device; a ``KEYPOINT`` array; or a CUDA int32 tensor (n, 18).  ``out``: a CUDA float32 tensor
        (n, 768) to fill -- usable as it is by ``DescriptorMatcher.set_descriptors``; without it a NumPy array comes back, or a new
        tensor when a tensor went in.  Process a long list in chunks: a million descriptors are 3 GB."""
        if keypoints is None:
            ptr, count, mem_in, keep = None, self._kp_count, capi.HOST, None
        else:
            ptr, count, mem_in, keep = self._records(keypoints, self.KEYPOINT, "describe")
            if mem_in == capi.DEVICE:
                self._adopt_stream_of(keypoints)
        if out is None and mem_in == capi.DEVICE:
            import torch
            out = torch.empty((count, self.DESCRIPTOR_LENGTH), dtype=torch.float32, device=keep.device)
        if out is None:
            out = np.zeros((count, self.DESCRIPTOR_LENGTH), np.float32)
        if tuple(out.shape) != (count, self.DESCRIPTOR_LENGTH):
            raise ValueError("describe: the output must have shape (%d, %d)" % (count, self.DESCRIPTOR_LENGTH))
        if _is_torch(out):
            optr, mem, _ = _buf(out)
        else:
            if out.dtype != np.float32 or not out.flags.c_contiguous:
                raise ValueError("describe: the output must be a contiguous float32 array")
            optr, mem = ctypes.c_void_p(out.ctypes.data), capi.HOST
        capi.check(capi.lib().oc_hip_sift3d_describe(self._h, ptr, count, mem_in, optr if count else None, mem))
        return out


class SIFT2DScaleSpace(_Handle):
    """SIFT2DScaleSpace() -- the detector of SIFT2D::compute (src/oc_sift.cpp:60-93): what cv::SIFT::detect does before it assigns
    orientations, for the cv::SIFT that SIFT2D creates from its Sift2dConfig (:22-30).  The 2x upscaled base, the Gaussian and DoG
    pyramids (``build``), and the located keypoints after the 26-neighbour extrema scan and the sub-pixel localisation with its
    contrast and edge rejections (``detect``), in the scan order of the extremum each one started from.  Images are (rows, cols)
    uint8 or float32 on the 0 ... 255 scale; a NumPy image is copied, a CUDA torch tensor is used in place by ``build``.  Both
    pyramids and the list stay on the device.  Orientation, descriptors, duplicate removal, ``n_features`` trimming and matching
    are not part of this engine."""

    KEYPOINT = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32), ("response", np.float32),
                         ("octave", np.int32), ("layer", np.int32), ("row", np.int32), ("col", np.int32),
                         ("xc", np.float32), ("xr", np.float32), ("xi", np.float32), ("packed_octave", np.int32)])
    LAYER = np.dtype([("dims", np.int32, 2), ("octave", np.int32), ("sigma", np.float32), ("radius", np.int32), ("threshold", np.int32)])
    GAUSSIAN, DOG = 0, 1

    def __init__(self, device=0):
        super().__init__(device)
        self._image = None
        capi.check(capi.lib().oc_hip_sift2d_create(int(device), ctypes.byref(self._h)))

    def set_tuning(self, key, value):
        """The keys every engine kind accepts; this engine has one arithmetic (``"arith_fma"`` = 1 is refused)."""
        capi.check(capi.lib().oc_hip_set_tuning(self._h, key.encode(), int(value)))

    def set_config(self, n_features=0, n_octave_layers=3, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6):
        """The members of Sift2dConfig; the defaults are SIFT2D::SIFT2D()'s (src/oc_sift.cpp:22-30).  ``n_features`` must be 0."""
        capi.check(capi.lib().oc_hip_sift2d_set_config(self._h, int(n_features), int(n_octave_layers), float(contrast_threshold),
                                                       float(edge_threshold), float(sigma)))

    def set_image(self, image):
        """``image``: (rows, cols) uint8 or float32, a NumPy array or a contiguous CUDA torch tensor."""
        if len(image.shape) != 2:
            raise ValueError("the image must have shape (rows, cols)")
        rows, cols = (int(v) for v in image.shape)
        if _is_torch(image):
            import torch
            if image.dtype not in (torch.uint8, torch.float32) or not image.is_contiguous() or not image.is_cuda:
                raise ValueError("a torch image must be a contiguous CUDA tensor of uint8 or float32 (pass NumPy arrays for host data)")
            self._adopt_stream_of(image)
            ptr, mem, keep, u8 = ctypes.c_void_p(image.data_ptr()), capi.DEVICE, image, image.dtype == torch.uint8
        else:
            u8 = np.asarray(image).dtype == np.uint8
            keep = np.ascontiguousarray(image, dtype=np.uint8 if u8 else np.float32)
            ptr, mem = ctypes.c_void_p(keep.ctypes.data), capi.HOST
        capi.check(capi.lib().oc_hip_sift2d_set_image(self._h, ptr, 0 if u8 else 1, cols, rows, mem))
        self._image = keep if mem == capi.DEVICE else None   # a device image is used in place: keep it alive

    def build(self):
        """The Gaussian and DoG pyramids of cv::SIFT::detect (src/oc_sift.cpp:86)."""
        capi.check(capi.lib().oc_hip_sift2d_build(self._h))

    def layers(self, pyramid):
        """One ``LAYER`` record per layer of the Gaussian (0) or DoG (1) pyramid; dims are (cols, rows)."""
        n, n_oct = ctypes.c_int(), ctypes.c_int()
        capi.check(capi.lib().oc_hip_sift2d_layer_count(self._h, int(pyramid), ctypes.byref(n), ctypes.byref(n_oct)))
        out = np.zeros(n.value, dtype=self.LAYER)
        for i in range(n.value):
            dims = (ctypes.c_int * 2)()
            octave, sigma, radius, threshold = ctypes.c_int(), ctypes.c_float(), ctypes.c_int(), ctypes.c_int()
            capi.check(capi.lib().oc_hip_sift2d_layer_info(self._h, int(pyramid), i, dims, ctypes.byref(octave), ctypes.byref(sigma),
                                                           ctypes.byref(radius), ctypes.byref(threshold)))
            out[i] = (tuple(dims), octave.value, sigma.value, radius.value, threshold.value)
        return out

    def layer(self, pyramid, index, out=None):
        """One layer as a (rows, cols) float32 array; ``out``: a CUDA torch tensor of that shape to fill instead."""
        dims = (ctypes.c_int * 2)()
        capi.check(capi.lib().oc_hip_sift2d_layer_info(self._h, int(pyramid), int(index), dims, None, None, None, None))
        shape = (dims[1], dims[0])
        if out is None:
            out = np.empty(shape, dtype=np.float32)
        elif tuple(out.shape) != shape:
            raise ValueError("layer: the output must have shape %r" % (shape,))
        if _is_torch(out):
            ptr, mem, _ = _buf(out)
        else:
            if out.dtype != np.float32 or not out.flags.c_contiguous:
                raise ValueError("layer: the output must be a contiguous float32 array")
            ptr, mem = ctypes.c_void_p(out.ctypes.data), capi.HOST
        capi.check(capi.lib().oc_hip_sift2d_get_layer(self._h, int(pyramid), int(index), ptr, mem))
        return out

    def keypoint_count(self):
        n = ctypes.c_size_t()
        capi.check(capi.lib().oc_hip_sift2d_keypoint_count(self._h, ctypes.byref(n)))
        return n.value

    def detect(self, on_device=False):
        """The located keypoints: a ``KEYPOINT`` array, or with ``on_device`` a CUDA int32 tensor (n, 12) of the records' words."""
        n = self.keypoint_count()
        got = ctypes.c_size_t()
        if on_device:
            import torch
            out = torch.empty((n, self.KEYPOINT.itemsize // 4), dtype=torch.int32, device="cuda:%d" % self._device)
            if n:
                capi.check(capi.lib().oc_hip_sift2d_detect(self._h, ctypes.c_void_p(out.data_ptr()), n, ctypes.byref(got), capi.DEVICE))
            return out
        out = np.empty(n, dtype=self.KEYPOINT)
        if n:
            capi.check(capi.lib().oc_hip_sift2d_detect(self._h, ctypes.c_void_p(out.ctypes.data), n, ctypes.byref(got), capi.HOST))
        return out


class SIFT3D:
    """SIFT3D() -- SIFT3D::compute (src/oc_sift.cpp:234-293) end to end on the GPU: two extractions (``SIFT3DScaleSpace``: pyramids,
    extrema, orientation, descriptors) and the brute-force matching of ``DescriptorMatcher``; descriptors go from one to the other
    as device blocks.  ``compute(ref, tar)`` returns the matched ``coor_img`` pairs, (n, 3) float32 (x, y, z) each, in the order
    monodirectionalMatch (default, as :285) or bidirectionalMatch gives them.  Volumes are (z, y, x) float32."""

    def __init__(self, device=0):
        self._device = int(device)
        self.extractor = SIFT3DScaleSpace(device)
        self.matcher = DescriptorMatcher(SIFT3DScaleSpace.DESCRIPTOR_LENGTH, 0.85, device)
        self.ref_keypoints = self.tar_keypoints = None

    def close(self):
        self.extractor.close()
        self.matcher.close()

    def set_config(self, **settings):
        """Any of n_octave_layers, min_dimension, alpha, sigma_source, sigma_base (``SIFT3DScaleSpace.set_config``) and beta, gamma,
        gradient_threshold, truncate_threshold (``set_feature_config``); what is not named takes the reference's default."""
        front = {k: settings.pop(k) for k in ("n_octave_layers", "min_dimension", "alpha", "sigma_source", "sigma_base") if k in settings}
        self.extractor.set_config(**front)
        self.extractor.set_feature_config(**settings)

    def set_physical_unit(self, unit_x, unit_y, unit_z):
        self.extractor.set_physical_unit(unit_x, unit_y, unit_z)

    def set_matching_ratio(self, ratio):
        self.matcher.set_ratio(ratio)

    def extract(self, volume):
        """(keypoints as a ``KEYPOINT`` array, descriptors as a CUDA tensor (n, 768)) of one volume"""
        import torch
        s = self.extractor
        s.set_volume(volume)
        s.build()
        kp = s.orient()
        desc = torch.empty((len(kp), s.DESCRIPTOR_LENGTH), dtype=torch.float32, device=torch.device("cuda", self._device))
        s.describe(None, out=desc)
        return kp, desc

    def compute(self, ref, tar, bidirectional=False):
        self.ref_keypoints, ref_desc = self.extract(ref)
        self.tar_keypoints, tar_desc = self.extract(tar)
        self.matcher.set_descriptors(0, ref_desc)
        self.matcher.set_descriptors(1, tar_desc)
        ri, ti = self.matcher.match(DescriptorMatcher.BIDIRECTIONAL if bidirectional else DescriptorMatcher.MONODIRECTIONAL)
        ri, ti = ri.cpu().numpy(), ti.cpu().numpy()
        return self.ref_keypoints["coor_img"][ri], self.tar_keypoints["coor_img"][ti]


class RegionFit:
    """RegionFit2D / RegionFit3D(neighbor_search_radius, neighbor_number_min, thread_number) -- src/oc_region_fit.h.

    ``set_neighbor(reliable)`` + ``prepare()`` build the neighbour search over the reliable POIs (their displacements
    are snapshotted at ``prepare``); ``compute(pois)`` gives every POI of a second queue the plane fitted through the
    reliable POIs around it as its deformation, with ``zncc = 0`` -- ready for another ICGN pass.  2D or 3D by the
    record size of the queues."""

    def __init__(self, neighbor_search_radius, neighbor_number_min, thread_number=1, device=0):
        self._h = ctypes.c_void_p()
        self.thread_number = thread_number
        self._device = int(device)
        self._radius, self._nmin = float(neighbor_search_radius), int(neighbor_number_min)
        self._reliable = None
        capi.check(capi.lib().oc_hip_region_fit_create(self._radius, self._nmin, device, ctypes.byref(self._h)))

    close = Strain.close
    __del__ = Strain.__del__
    set_stream = Strain.set_stream
    _adopt_stream_of = _Engine._adopt_stream_of
    _stream_pinned = False
    _auto_stream = None
    _on_private_stream = True
    synchronize = Strain.synchronize
    profile_enable = Strain.profile_enable
    profile_reset = Strain.profile_reset
    profile_read = Strain.profile_read

    def set_search_radius(self, neighbor_search_radius):
        capi.check(capi.lib().oc_hip_region_fit_set(self._h, float(neighbor_search_radius), self._nmin))
        self._radius = float(neighbor_search_radius)

    def set_neighbor_min(self, neighbor_number_min):
        capi.check(capi.lib().oc_hip_region_fit_set(self._h, self._radius, int(neighbor_number_min)))
        self._nmin = int(neighbor_number_min)

    def set_neighbor(self, reliable_pois):
        self._reliable = reliable_pois

    def prepare(self):
        if self._reliable is None:
            raise ValueError("RegionFit.prepare: call set_neighbor(reliable_pois) first")
        self._adopt_stream_of(self._reliable)
        p, n, stride, ndim, mem = Strain._queue(self._reliable)
        capi.check(capi.lib().oc_hip_region_fit_prepare(self._h, p, n, stride, ndim, mem))

    def compute(self, pois):
        self._adopt_stream_of(pois)
        p, n, stride, ndim, mem = Strain._queue(pois)
        capi.check(capi.lib().oc_hip_region_fit_compute(self._h, p, n, stride, ndim, mem))
        return pois


class _FeatureAffine(_Handle):
    """What FeatureAffine2D and FeatureAffine3D share (src/oc_feature_affine.h): the keypoint-guided RANSAC affine initial
    guess.  ``set_keypoint_pair(ref_kp, tar_kp)`` takes the matched keypoints ((m, ndim) float32, NumPy or CUDA tensor;
    copied), ``prepare()`` builds the neighbour search over the reference keypoints, ``compute(pois)`` writes the
    first-order deformation, ``result.iteration`` (trials), ``result.feature`` (inliers; POI3D: float 21) and ``zncc``
    (0, -1 too few keypoints, -2 no consensus) of every POI in place.  Deterministic: the samples come from a counter-based
    generator keyed by ``set_seed`` and the POI's coordinates."""
    _ndim = 0

    def _create(self, radii, thread_number, device):
        super().__init__(device)
        self.thread_number = thread_number
        capi.check(capi.lib().oc_hip_feature_affine_create(self._ndim, int(radii[0]), int(radii[1]), int(radii[2]), int(device),
                                                           ctypes.byref(self._h)))
        r2 = sum(int(r) * int(r) for r in radii[:self._ndim])
        self._radius = float(np.sqrt(np.float32(r2)))

    def get_ransac_config(self):
        return dict(self._ransac)

    def get_search_radius(self):
        return self._radius

    def get_neighbor_min(self):
        return self._nmin

    def set_search(self, neighbor_search_radius, neighbor_number_min):
        capi.check(capi.lib().oc_hip_feature_affine_set_search(self._h, float(neighbor_search_radius), int(neighbor_number_min)))
        self._radius, self._nmin = float(np.float32(neighbor_search_radius)), int(neighbor_number_min)

    def set_ransac_config(self, trial_number, sample_number, error_threshold):
        """RansacConfig: trial_number (1 ... 1024), sample_mumber (ndim + 1 ... 8), error_threshold."""
        capi.check(capi.lib().oc_hip_feature_affine_set_ransac(self._h, int(trial_number), int(sample_number), float(error_threshold)))
        self._ransac = dict(trial_number=int(trial_number), sample_number=int(sample_number), error_threshold=float(error_threshold))

    def set_seed(self, seed):
        capi.check(capi.lib().oc_hip_feature_affine_set_seed(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF))

    def set_tuning(self, key, value):
        capi.check(capi.lib().oc_hip_set_tuning(self._h, key.encode(), int(value)))

    def _points(self, x, what):
        if not _is_torch(x):
            x = np.ascontiguousarray(x, dtype=np.float32)
        elif not x.is_contiguous():
            x = x.contiguous()
        if len(x.shape) != 2 or x.shape[1] != self._ndim:
            raise ValueError("%s: keypoints must have shape (count, %d)" % (what, self._ndim))
        return x

    def set_keypoint_pair(self, ref_kp, tar_kp):
        ref_kp, tar_kp = self._points(ref_kp, "set_keypoint_pair"), self._points(tar_kp, "set_keypoint_pair")
        if ref_kp.shape[0] != tar_kp.shape[0] or _is_torch(ref_kp) != _is_torch(tar_kp):
            raise ValueError("set_keypoint_pair: the two sides differ in length or memory space")
        self._adopt_stream_of(ref_kp)
        pr, mem, _ = _buf(ref_kp)
        pt, _, _ = _buf(tar_kp)
        capi.check(capi.lib().oc_hip_feature_affine_set_keypoints(self._h, pr, pt, ref_kp.shape[0], mem))

    def set_matched_pairs(self, ref_kp, tar_kp, ref_idx, tar_idx):
        """The pairs ``DescriptorMatcher.match`` returned, gathered on the device: pair k is (ref_kp[ref_idx[k]],
        tar_kp[tar_idx[k]]).  CUDA tensors: keypoints (count, ndim) float32, indices int32.  A negative index is refused
        (the engine then holds no keypoints); indices are not checked against the keypoint counts."""
        import torch
        ref_kp, tar_kp = self._points(ref_kp, "set_matched_pairs"), self._points(tar_kp, "set_matched_pairs")
        for t in (ref_kp, tar_kp, ref_idx, tar_idx):
            if not _is_torch(t) or not t.is_cuda:
                raise ValueError("set_matched_pairs: every array is a CUDA tensor")
        if ref_idx.dtype != torch.int32 or tar_idx.dtype != torch.int32 or ref_idx.shape != tar_idx.shape or ref_idx.dim() != 1:
            raise ValueError("set_matched_pairs: the index lists are int32 vectors of one length")
        ref_idx, tar_idx = ref_idx.contiguous(), tar_idx.contiguous()
        self._adopt_stream_of(ref_kp)
        capi.check(capi.lib().oc_hip_feature_affine_set_matched(self._h, ctypes.c_void_p(ref_kp.data_ptr()), ctypes.c_void_p(tar_kp.data_ptr()),
                                                                ctypes.c_void_p(ref_idx.data_ptr()), ctypes.c_void_p(tar_idx.data_ptr()),
                                                                ref_idx.shape[0], capi.DEVICE))

    def prepare(self):
        capi.check(capi.lib().oc_hip_feature_affine_prepare(self._h))

    def compute(self, pois):
        self._adopt_stream_of(pois)
        p, n, stride, mem, _ = self._rows(pois, capi.POI2D_FLOATS if self._ndim == 2 else capi.POI3D_FLOATS, "compute")
        capi.check(capi.lib().oc_hip_feature_affine_compute(self._h, p, n, stride, mem))
        return pois


class FeatureAffine2D(_FeatureAffine):
    """FeatureAffine2D(radius_x, radius_y, thread_number) -- src/oc_feature_affine.h:37-70, src/oc_feature_affine.cpp:34-55."""
    _ndim = 2

    def __init__(self, radius_x, radius_y, thread_number=1, device=0):
        self._create((radius_x, radius_y, 0), thread_number, device)
        self._nmin = 7
        self._ransac = dict(trial_number=20, sample_number=3, error_threshold=1.5)
        self._adjust = (14, 10)
        self._size = None
        self._adaptive = False

    def set_images(self, height, width):
        """The reference reads ref_img->width / height in self-adaptive mode (:130-133): the size is all this engine needs."""
        self._size = (int(height), int(width))
        self._push_adaptive()

    def set_self_adaptive(self, is_self_adaptive):
        self._adaptive = bool(is_self_adaptive)
        self._push_adaptive()

    def set_subset_adjustment(self, feature_min, radius_min):
        self._adjust = (int(feature_min), int(radius_min))
        self._push_adaptive()

    def _push_adaptive(self):
        if self._adaptive and self._size is None:
            return  # (compute refuses below until the size is known)
        h, w = self._size or (0, 0)
        capi.check(capi.lib().oc_hip_feature_affine_set_self_adaptive(self._h, 1 if self._adaptive else 0, self._adjust[0], self._adjust[1], w, h))

    def compute(self, pois):
        if self._adaptive and self._size is None:
            raise ValueError("FeatureAffine2D: self-adaptive subsets need set_images(height, width)")
        return super().compute(pois)


class FeatureAffine3D(_FeatureAffine):
    """FeatureAffine3D(radius_x, radius_y, radius_z, thread_number) -- src/oc_feature_affine.h:77-106, src/oc_feature_affine.cpp:357-374."""
    _ndim = 3

    def __init__(self, radius_x, radius_y, radius_z, thread_number=1, device=0):
        self._create((radius_x, radius_y, radius_z), thread_number, device)
        self._nmin = 16
        self._ransac = dict(trial_number=32, sample_number=4, error_threshold=3.2)


class FFTCC3D(_Engine):
    """FFTCC3D(rx, ry, rz, thread_number) -- src/oc_fftcc.h:75-89."""
    _ndim = 3

    def __init__(self, subset_radius_x, subset_radius_y, subset_radius_z, thread_number=1, device=0):
        super().__init__(device)
        self.thread_number = thread_number
        capi.check(capi.lib().oc_hip_fftcc3d_create(subset_radius_x, subset_radius_y, subset_radius_z, device,
                                                    ctypes.byref(self._h)))


class ICGN3D1(_Engine, _IcgnMixin):
    """ICGN3D1(rx, ry, rz, conv_criterion, stop_condition, thread_number) -- src/oc_icgn.h:155-180."""
    _ndim = 3

    def __init__(self, subset_radius_x, subset_radius_y, subset_radius_z, conv_criterion, stop_condition,
                 thread_number=1, device=0):
        super().__init__(device)
        self.thread_number = thread_number
        capi.check(capi.lib().oc_hip_icgn3d1_create(subset_radius_x, subset_radius_y, subset_radius_z, conv_criterion,
                                                    stop_condition, device, ctypes.byref(self._h)))


def compute_chain(engines, pois):
    """Several engines over ONE queue, in order (``oc_hip_compute_chain``): ``compute_chain([fftcc, icgn], pois)`` does what
    ``fftcc.compute(pois); icgn.compute(pois)`` does -- same bits -- but a host (NumPy) queue crosses PCIe once in each
    direction instead of once per engine."""
    engines = list(engines)
    if not engines:
        raise ValueError("compute_chain needs at least one engine")
    floats = capi.POI2D_FLOATS if engines[0]._ndim == 2 else capi.POI3D_FLOATS
    for e in engines:
        e._adopt_stream_of(pois)
    if _is_torch(pois):
        p, mem, _ = _buf(pois)
        n, stride = pois.shape[0], pois.stride(0) * 4
        if pois.shape[1] < floats:
            raise ValueError("POI records need %d floats" % floats)
    else:
        if pois.dtype != np.float32 or not pois.flags.c_contiguous or pois.ndim != 2 or pois.shape[1] < floats:
            raise ValueError("pois must be a C-contiguous float32 array of shape (n, >=%d)" % floats)
        p, mem = ctypes.c_void_p(pois.ctypes.data), capi.HOST
        n, stride = pois.shape[0], pois.strides[0]
    handles = (ctypes.c_void_p * len(engines))(*[e._h for e in engines])
    capi.check(capi.lib().oc_hip_compute_chain(handles, len(engines), p, n, stride, mem))
    return pois


def make_pois2d(xs, ys):
    """Zero-initialised POI2D records (POI2D ctor, src/oc_poi.h:108-135)."""
    xs = np.asarray(xs, dtype=np.float32).ravel()
    pois = np.zeros((xs.size, capi.POI2D_FLOATS), dtype=np.float32)
    pois[:, 0] = xs
    pois[:, 1] = np.asarray(ys, dtype=np.float32).ravel()
    return pois


def make_pois3d(xs, ys, zs):
    xs = np.asarray(xs, dtype=np.float32).ravel()
    pois = np.zeros((xs.size, capi.POI3D_FLOATS), dtype=np.float32)
    pois[:, 0] = xs
    pois[:, 1] = np.asarray(ys, dtype=np.float32).ravel()
    pois[:, 2] = np.asarray(zs, dtype=np.float32).ravel()
    return pois
