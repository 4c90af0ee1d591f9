"""ctypes binding of include/homulator_hip.h (libhomulator_hip.so).  No CPU fallback: a missing library or a
machine without a HIP device is an error, never a silent detour."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HOMULATOR_HIP_LIB") or os.path.join(_HERE, "lib", "libhomulator_hip.so")  # override: A/B builds
# the two arithmetic back-ends libhomulator_hip.so maps from its own directory (hm_dispatch.cpp): word-wise Montgomery for chains of
# primes h 2^32 + 1 (the default), Shoup / Barrett for any other NTT-friendly chain below 2^60
BACKEND_LIBS = ("libhm_m32.so", "libhm_gen.so")

OP_MUL, OP_MAC2, OP_MAC_ADD, OP_ADD, OP_SUB, OP_MUL_CONST, OP_SUB_SCALE, OP_COPY, OP_SUB_SCALE_ADD, OP_ADD_CONST = range(10)
NO_LIMB = 0xFFFFFFFF   # HM_NO_LIMB: "this entry has no such operand" in an optional limb list
LINCOMB_MULTI_MAX_OUT = 16   # HM_LINCOMB_MULTI_MAX_OUT: outputs per entry of hm_lincomb_multi
LINCOMB_MULTI_TILE = 4       # HM_LINCOMB_MULTI_TILE: outputs a record of hm_lincomb_multi serves (the inputs are read once per tile)
LINTRANS_MULTI_TILE = 2   # HM_IP_LINTRANS_MULTI_TILE: outputs a workgroup of hm_inner_product_lintrans_multi serves

# every symbol include/homulator_hip.h declares
SYMBOLS = [
    "hm_create", "hm_destroy", "hm_last_error", "hm_version", "hm_get_modulus", "hm_get_psi", "hm_malloc", "hm_free",
    "hm_memcpy_h2d", "hm_memcpy_d2h", "hm_memcpy_d2d", "hm_sync", "hm_stream", "hm_wait_for", "hm_ntt", "hm_ntt_sub_scale", "hm_ntt_mix_sub_scale", "hm_tensor", "hm_inner_product", "hm_automorph", "hm_ewe",
    "hm_bconv", "hm_bconv_batch", "hm_bconv_consts", "hm_fill_uniform", "hm_timer_start", "hm_timer_stop", "hm_comm_unique_id", "hm_comm_init_rccl", "hm_comm_init_external",
    "hm_capture_begin", "hm_capture_end", "hm_graph_launch", "hm_graph_destroy", "hm_comm_info", "hm_slice_rows", "hm_limbs_to_slices", "hm_slices_to_limbs", "hm_replicate_limbs",
    "hm_set_option", "hm_get_counter", "hm_ntt_inner_product", "hm_exchange_stream", "hm_exchange_mark", "hm_exchange_wait",
    "hm_bconv_col", "hm_limbs_to_colslices", "hm_colslices_to_limbs", "hm_ntt_second_pass", "hm_ntt_ex", "hm_capability", "hm_inner_product_ex",
    "hm_inner_product_hoisted", "hm_inner_product_lintrans", "hm_inner_product_rotsum", "hm_inner_product_lintrans_multi",
    "hm_tensor_dot", "hm_inner_product_lintrans_id", "hm_inner_product_rotsum_init", "hm_ntt_mix_sub_scale_mul", "hm_ntt_mul",
    "hm_ntt_lift", "hm_tensor_square", "hm_lincomb", "hm_tensor_muladd", "hm_reim_split", "hm_clincomb", "hm_plincomb",
    "hm_tensor_dotadd", "hm_lincomb_multi", "hm_encode", "hm_decode",
]


class hm_ntt_fused_desc(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("in_limbs", C.c_void_p), ("mix", C.c_void_p), ("mix_limbs", C.c_void_p), ("mix_k", C.c_void_p),
                ("minuend", C.c_void_p), ("minuend_limbs", C.c_void_p), ("addend", C.c_void_p), ("addend_limbs", C.c_void_p),
                ("addend_k", C.c_void_p), ("out", C.c_void_p), ("out_limbs", C.c_void_p), ("mod_ids", C.c_void_p), ("n", C.c_uint32),
                ("k", C.c_void_p), ("conv", C.c_void_p), ("n_conv", C.c_uint32), ("addend_galois", C.c_void_p)]


class hm_ip_desc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_limbs", C.c_void_p), ("y", C.c_void_p), ("y_limbs", C.c_void_p), ("out", C.c_void_p), ("out_limbs", C.c_void_p),
                ("mod_ids", C.c_void_p), ("n", C.c_uint32), ("n_terms", C.c_uint32), ("n_out", C.c_uint32), ("x_galois", C.c_uint32)]


class hm_ip_hoisted_desc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_limbs", C.c_void_p), ("y", C.c_void_p), ("y_limbs", C.c_void_p), ("out", C.c_void_p), ("out_limbs", C.c_void_p),
                ("mod_ids", C.c_void_p), ("n", C.c_uint32), ("n_terms", C.c_uint32), ("n_rot", C.c_uint32), ("galois", C.c_void_p)]


class hm_ip_lintrans_desc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_limbs", C.c_void_p), ("y", C.c_void_p), ("y_limbs", C.c_void_p), ("pt", C.c_void_p), ("pt_limbs", C.c_void_p),
                ("addend", C.c_void_p), ("addend_limbs", C.c_void_p), ("out", C.c_void_p), ("out_limbs", C.c_void_p),
                ("addend_out", C.c_void_p), ("addend_out_limbs", C.c_void_p), ("mod_ids", C.c_void_p),
                ("n", C.c_uint32), ("n_terms", C.c_uint32), ("n_rot", C.c_uint32), ("galois", C.c_void_p)]


class hm_ip_lintrans_multi_desc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_limbs", C.c_void_p), ("y", C.c_void_p), ("y_limbs", C.c_void_p), ("pt", C.c_void_p), ("pt_limbs", C.c_void_p),
                ("addend", C.c_void_p), ("addend_limbs", C.c_void_p), ("out", C.c_void_p), ("out_limbs", C.c_void_p),
                ("addend_out", C.c_void_p), ("addend_out_limbs", C.c_void_p), ("mod_ids", C.c_void_p),
                ("n", C.c_uint32), ("n_terms", C.c_uint32), ("n_rot", C.c_uint32), ("n_out", C.c_uint32), ("galois", C.c_void_p)]


class hm_ip_lintrans_id_desc(C.Structure):
    _fields_ = [("sums", hm_ip_lintrans_multi_desc), ("id_pt_limbs", C.c_void_p), ("addend1", C.c_void_p), ("addend1_limbs", C.c_void_p),
                ("addend1_out", C.c_void_p), ("addend1_out_limbs", C.c_void_p)]


class hm_ip_rotsum_desc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_limbs", C.c_void_p), ("y", C.c_void_p), ("y_limbs", C.c_void_p),
                ("addend", C.c_void_p), ("addend_limbs", C.c_void_p), ("out", C.c_void_p), ("out_limbs", C.c_void_p),
                ("addend_out", C.c_void_p), ("addend_out_limbs", C.c_void_p), ("mod_ids", C.c_void_p),
                ("n", C.c_uint32), ("n_terms", C.c_uint32), ("n_ct", C.c_uint32), ("galois", C.c_void_p)]


class hm_ip_rotsum_init_desc(C.Structure):
    _fields_ = [("sum", hm_ip_rotsum_desc), ("init", C.c_void_p), ("init_limbs", C.c_void_p), ("addend_init_limbs", C.c_void_p)]


class hm_ntt_ip_desc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_limbs", C.c_void_p), ("x_is_coeff", C.c_void_p), ("hand", C.c_void_p), ("hand_limbs", C.c_void_p),
                ("y", C.c_void_p), ("y_limbs", C.c_void_p), ("out", C.c_void_p), ("out_limbs", C.c_void_p), ("mod_ids", C.c_void_p),
                ("n", C.c_uint32), ("n_terms", C.c_uint32), ("n_out", C.c_uint32), ("conv", C.c_void_p), ("n_conv", C.c_uint32),
                ("out_inverse", C.c_void_p), ("x_galois", C.c_uint32)]


class hm_bconv_desc(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("in_limbs", C.c_void_p), ("in_ids", C.c_void_p), ("n_in", C.c_uint32),
                ("out", C.c_void_p), ("out_limbs", C.c_void_p), ("out_ids", C.c_void_p), ("n_out", C.c_uint32),
                ("log_len", C.c_uint32), ("sub_from", C.c_void_p), ("sub_from_limbs", C.c_void_p), ("add", C.c_void_p), ("add_limbs", C.c_void_p),
                ("sub_k", C.c_void_p), ("in_packed", C.c_uint32)]


class hm_ntt_desc(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("in_limbs", C.c_void_p), ("out", C.c_void_p), ("out_limbs", C.c_void_p), ("mod_ids", C.c_void_p), ("n", C.c_uint32),
                ("inverse", C.c_int), ("scale", C.c_void_p), ("second_pass_only", C.c_int), ("out_packed", C.c_void_p),
                ("in_galois", C.c_void_p)]


class hm_ntt_fused_mul_desc(C.Structure):
    _fields_ = [("t", hm_ntt_fused_desc), ("minuend_b", C.c_void_p), ("minuend_b_limbs", C.c_void_p)]


class hm_ntt_mul_desc(C.Structure):
    _fields_ = [("t", hm_ntt_desc), ("in_b", C.c_void_p), ("in_b_limbs", C.c_void_p)]


class hm_ntt_lift_desc(C.Structure):
    _fields_ = [("t", hm_ntt_desc), ("src_mod_ids", C.c_void_p)]


class hm_params(C.Structure):
    _fields_ = [("logN", C.c_uint32), ("L", C.c_uint32), ("K", C.c_uint32), ("device", C.c_int32),
                ("q", C.c_void_p), ("p", C.c_void_p), ("psi", C.c_void_p)]


_lib = None


def load():
    """Load the HIP backend.  Raises if it has not been built (run `python -c 'import __graft_entry__ as g; g.build()'`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                          "(make -C homulator_amd/csrc); homulator_amd has no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    L.hm_create.argtypes = [C.POINTER(vp), C.POINTER(hm_params)]
    L.hm_destroy.argtypes = [vp]
    L.hm_last_error.restype = C.c_char_p
    L.hm_last_error.argtypes = [vp]
    L.hm_version.restype = C.c_char_p
    L.hm_get_modulus.argtypes = [vp, u32, C.POINTER(u64)]
    L.hm_get_psi.argtypes = [vp, u32, C.POINTER(u64)]
    L.hm_malloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.hm_free.argtypes = [vp, vp]
    L.hm_memcpy_h2d.argtypes = [vp, vp, vp, C.c_size_t]
    L.hm_memcpy_d2h.argtypes = [vp, vp, vp, C.c_size_t]
    L.hm_memcpy_d2d.argtypes = [vp, vp, vp, C.c_size_t]
    L.hm_sync.argtypes = [vp]
    L.hm_stream.restype = vp
    L.hm_stream.argtypes = [vp]
    L.hm_wait_for.argtypes = [vp, vp]
    L.hm_ntt.argtypes = [vp, vp, vp, vp, vp, vp, u32, i32, vp]
    L.hm_ntt_second_pass.argtypes = [vp, vp, vp, vp, u32, i32, vp]
    L.hm_ntt_ex.argtypes = [vp, C.POINTER(hm_ntt_desc)]
    L.hm_inner_product_ex.argtypes = [vp, C.POINTER(hm_ip_desc)]
    L.hm_inner_product_hoisted.argtypes = [vp, C.POINTER(hm_ip_hoisted_desc)]
    L.hm_inner_product_lintrans.argtypes = [vp, C.POINTER(hm_ip_lintrans_desc)]
    L.hm_inner_product_rotsum.argtypes = [vp, C.POINTER(hm_ip_rotsum_desc)]
    L.hm_inner_product_lintrans_multi.argtypes = [vp, C.POINTER(hm_ip_lintrans_multi_desc)]
    L.hm_inner_product_rotsum_init.argtypes = [vp, C.POINTER(hm_ip_rotsum_init_desc)]
    L.hm_inner_product_lintrans_id.argtypes = [vp, C.POINTER(hm_ip_lintrans_id_desc)]
    L.hm_ntt_sub_scale.argtypes = [vp] + [vp] * 9 + [u32, vp]
    L.hm_ntt_mix_sub_scale.argtypes = [vp, C.POINTER(hm_ntt_fused_desc)]
    L.hm_ntt_mix_sub_scale_mul.argtypes = [vp, C.POINTER(hm_ntt_fused_mul_desc)]
    L.hm_ntt_mul.argtypes = [vp, C.POINTER(hm_ntt_mul_desc)]
    L.hm_ntt_lift.argtypes = [vp, C.POINTER(hm_ntt_lift_desc)]
    L.hm_encode.argtypes = [vp, vp, u32, C.c_double, vp, vp, u32, vp, vp, vp, u32]
    L.hm_decode.argtypes = [vp, vp, vp, u32, C.c_double, vp, vp, vp, u32]
    L.hm_tensor.argtypes = [vp] + [vp] * 15 + [u32]
    L.hm_tensor_dot.argtypes = [vp] + [vp] * 15 + [u32, u32]
    L.hm_tensor_square.argtypes = [vp] + [vp] * 11 + [u32, vp, vp]
    L.hm_lincomb.argtypes = [vp] + [vp] * 5 + [u32, u32, vp, vp]
    L.hm_lincomb_multi.argtypes = [vp] + [vp] * 5 + [u32, u32, u32, vp, vp]
    L.hm_tensor_muladd.argtypes = [vp] + [vp] * 18 + [u32, u32, vp, vp, vp]
    L.hm_reim_split.argtypes = [vp] + [vp] * 9 + [u32]
    L.hm_clincomb.argtypes = [vp] + [vp] * 5 + [u32, u32, vp, vp, vp, vp]
    L.hm_plincomb.argtypes = [vp] + [vp] * 11 + [u32, u32]
    L.hm_tensor_dotadd.argtypes = [vp] + [vp] * 18 + [u32, u32, u32, vp, vp, vp]
    L.hm_inner_product.argtypes = [vp] + [vp] * 7 + [u32, u32, u32]
    L.hm_automorph.argtypes = [vp, vp, vp, vp, vp, u32, u32]
    L.hm_ewe.argtypes = [vp, i32] + [vp] * 11 + [u32, vp]
    L.hm_bconv.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, u32]
    L.hm_bconv_batch.argtypes = [vp, C.POINTER(hm_bconv_desc), u32]
    L.hm_bconv_consts.argtypes = [vp, vp, u32, vp, u32, vp, vp]
    L.hm_fill_uniform.argtypes = [vp, vp, vp, vp, u32, u64]
    L.hm_ntt_inner_product.argtypes = [vp, C.POINTER(hm_ntt_ip_desc)]
    L.hm_set_option.argtypes = [vp, C.c_char_p, u64]
    L.hm_get_counter.argtypes = [vp, C.c_char_p, C.POINTER(u64)]
    L.hm_capability.argtypes = [u32, C.c_char_p, C.POINTER(u64)]
    L.hm_comm_init_external.argtypes = [vp, i32, i32, vp, vp]
    L.hm_slice_rows.argtypes = [vp, u32, u32, vp]
    L.hm_limbs_to_slices.argtypes = [vp, vp, vp, vp, u32, vp]
    L.hm_slices_to_limbs.argtypes = [vp, vp, vp, vp, vp, u32]
    L.hm_limbs_to_colslices.argtypes = [vp, vp, vp, vp, u32, vp]
    L.hm_colslices_to_limbs.argtypes = [vp, vp, vp, vp, vp, u32]
    L.hm_replicate_limbs.argtypes = [vp, vp, vp, vp, u32]
    L.hm_bconv_col.argtypes = [vp, C.POINTER(hm_bconv_desc), u32, u32, u32]
    L.hm_timer_start.argtypes = [vp]
    L.hm_timer_stop.argtypes = [vp, C.POINTER(u64)]
    _lib = L
    return L


class HmError(RuntimeError):
    pass


def capability(logN, name):
    """the back-end's capability table (homulator_amd/csrc/hm_caps.h) for ring size 2^logN: needs no context and no GPU"""
    v = C.c_uint64()
    if load().hm_capability(int(logN), name.encode(), C.byref(v)) != 0:
        raise HmError(f"hm_capability: unknown capability {name}")
    return v.value


def _u32(a):
    if a is None:
        return None, None
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.uint32))
    return arr, arr.ctypes.data_as(C.c_void_p)


def _dev_ptr(x):
    """the device address of a DeviceBuf (`.ptr`) or of anything that has `data_ptr()` (a torch tensor on the GPU)"""
    return x.ptr if hasattr(x, "ptr") else x.data_ptr()


def _on_device(x):
    """a DeviceBuf, or an object with data_ptr(); one that says it is not on the GPU (a CPU torch tensor: is_cuda False) is refused, since its host
    address would reach the kernels"""
    if hasattr(x, "ptr"):
        return True
    if not hasattr(x, "data_ptr"):
        return False
    if not getattr(x, "is_cuda", True):
        raise ValueError("a tensor with data_ptr() must be on the GPU (move it there, or pass a numpy array)")
    return True


def _u64(a):
    if a is None:
        return None, None
    arr = np.ascontiguousarray(np.asarray([int(x) for x in a], dtype=np.uint64))
    return arr, arr.ctypes.data_as(C.c_void_p)


class DeviceBuf:
    """[n_limbs][N] uint64 words in HBM, limb-major (a plain hipMalloc'd pointer)."""

    def __init__(self, ctx, n_limbs):
        self.ctx, self.n_limbs = ctx, n_limbs
        p = C.c_void_p()
        ctx._ck(ctx.L.hm_malloc(ctx.h, 8 * ctx.N * n_limbs, C.byref(p)))
        self.ptr = p.value

    def limb_ptr(self, limb):
        return self.ptr + 8 * self.ctx.N * limb

    def upload(self, arr, limb0=0):
        a = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, self.ctx.N)
        assert limb0 + a.shape[0] <= self.n_limbs
        self.ctx._ck(self.ctx.L.hm_memcpy_h2d(self.ctx.h, self.limb_ptr(limb0), a.ctypes.data_as(C.c_void_p), a.nbytes))
        return self

    def download(self, limb0=0, n=None):
        n = self.n_limbs - limb0 if n is None else n
        out = np.empty((n, self.ctx.N), dtype=np.uint64)
        self.ctx._ck(self.ctx.L.hm_memcpy_d2h(self.ctx.h, out.ctypes.data_as(C.c_void_p), self.limb_ptr(limb0), out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.ctx.L.hm_free(self.ctx.h, self.ptr)
            self.ptr = None


class Context:
    """One GPU, one parameter set.  Thin, 1:1 with the C ABI."""

    def __init__(self, logN, L, K, device=0, q=None, p=None):
        """q / p: the L chain moduli and the K special moduli (distinct primes = 1 mod 2N below 2^60; hm_create runs them on the
        word-wise Montgomery back-end if they all are h 2^32 + 1, on the generic one otherwise); default: the library's own chain"""
        self.L = load()
        self.h = C.c_void_p()
        qa = None if q is None else np.ascontiguousarray(np.asarray(q, dtype=np.uint64))
        pa = None if p is None else np.ascontiguousarray(np.asarray(p, dtype=np.uint64))
        if (qa is not None and len(qa) != L) or (pa is not None and len(pa) != K):
            raise ValueError("q needs L entries and p needs K")
        prm = hm_params(logN, L, K, device, None if qa is None else qa.ctypes.data_as(C.c_void_p), None if pa is None else pa.ctypes.data_as(C.c_void_p), None)
        st = self.L.hm_create(C.byref(self.h), C.byref(prm))
        if st != 0:
            raise HmError(f"hm_create failed ({st}): {self.L.hm_last_error(None).decode()}")
        self.logN, self.N, self.nQ, self.K = logN, 1 << logN, L, K
        self.chain = None if qa is None else [int(x) for x in qa] + ([] if pa is None else [int(x) for x in pa])
        q = C.c_uint64()
        self.moduli = []
        for m in range(L + K):
            self._ck(self.L.hm_get_modulus(self.h, m, C.byref(q)))
            self.moduli.append(q.value)

    def _ck(self, st):
        if st != 0:
            raise HmError(f"hm error {st}: {self.L.hm_last_error(self.h).decode()}")

    def close(self):
        if self.h:
            self.L.hm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def alloc(self, n_limbs):
        return DeviceBuf(self, n_limbs)

    def from_host(self, arr):
        a = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, self.N)
        return self.alloc(a.shape[0]).upload(a)

    def sync(self):
        self._ck(self.L.hm_sync(self.h))

    def ext_ids(self, ell):
        return list(range(ell)) + [self.nQ + i for i in range(self.K)]

    # ---- compute calls (device pointers + limb lists)
    def ntt(self, src, dst, mod_ids, inverse=False, in_limbs=None, out_limbs=None, scale=None, out_packed=None, in_galois=None):
        """out_packed (inverse only): per limb, store the split-30 packed form the base conversions take with in_packed (hm_ntt_ex);
        in_galois (inverse only): per limb, read the input through the automorphism X -> X^g (hm_ntt_ex)"""
        n = len(mod_ids)
        k1, pi = _u32(in_limbs)
        k2, po = _u32(out_limbs)
        k3, pm = _u32(mod_ids)
        k4, ps = _u64(scale)
        if out_packed is None and in_galois is None:
            self._ck(self.L.hm_ntt(self.h, src.ptr, pi, dst.ptr, po, pm, n, 1 if inverse else 0, ps))
            return
        pk = None if out_packed is None else np.ascontiguousarray(np.asarray(out_packed, dtype=np.uint8))
        k5, pg = _u32(in_galois)
        d = hm_ntt_desc(src.ptr, pi, dst.ptr, po, pm, n, 1 if inverse else 0, ps, 0, None if pk is None else pk.ctypes.data_as(C.c_void_p), pg)
        self._ck(self.L.hm_ntt_ex(self.h, C.byref(d)))

    def ntt_mul(self, src, in_b, dst, mod_ids, in_limbs=None, in_b_limbs=None, out_limbs=None, scale=None, out_packed=None):
        """dst = INTT(src (.) in_b) * N^-1 [* scale]: the product is formed while the first pass loads (hm_ntt_mul: the inverse transform)"""
        keep = [_u32(x) for x in (in_limbs, out_limbs, mod_ids, in_b_limbs)]
        k4, ps = _u64(scale)
        pk = None if out_packed is None else np.ascontiguousarray(np.asarray(out_packed, dtype=np.uint8))
        d = hm_ntt_mul_desc(hm_ntt_desc(src.ptr, keep[0][1], dst.ptr, keep[1][1], keep[2][1], len(mod_ids), 1, ps, 0,
                                        None if pk is None else pk.ctypes.data_as(C.c_void_p), None), in_b.ptr, keep[3][1])
        self._ck(self.L.hm_ntt_mul(self.h, C.byref(d)))

    def ntt_lift(self, src, dst, mod_ids, src_mod_ids, in_limbs=None, out_limbs=None, **refused):
        """dst_i = NTT_{mod_ids[i]}(centre_{src_mod_ids[i]}(src_i) mod q_{mod_ids[i]}): the stored coefficients of another modulus are centred and
        reduced while the first pass loads (hm_ntt_lift: ModRaise).  `refused`: hm_ntt_desc fields the call does not serve (inverse,
        second_pass_only, in_galois, scale, out_packed), passed through so that the refusal is the library's"""
        keep = [_u32(x) for x in (in_limbs, out_limbs, mod_ids, src_mod_ids, refused.get("in_galois"))]
        k4, ps = _u64(refused.get("scale"))
        pk = refused.get("out_packed")
        pk = None if pk is None else np.ascontiguousarray(np.asarray(pk, dtype=np.uint8))
        d = hm_ntt_lift_desc(hm_ntt_desc(src.ptr, keep[0][1], dst.ptr, keep[1][1], keep[2][1], len(mod_ids), 1 if refused.get("inverse") else 0, ps,
                                         1 if refused.get("second_pass_only") else 0, None if pk is None else pk.ctypes.data_as(C.c_void_p),
                                         keep[4][1]), keep[3][1])
        self._ck(self.L.hm_ntt_lift(self.h, C.byref(d)))

    def ntt_sub_scale(self, src, minuend, out, mod_ids, k, addend=None, in_limbs=None, minuend_limbs=None, addend_limbs=None,
                      out_limbs=None):
        keep = [_u32(x) for x in (in_limbs, minuend_limbs, addend_limbs, out_limbs, mod_ids)]
        kk, pk = _u64(k)
        self._ck(self.L.hm_ntt_sub_scale(self.h, src.ptr, keep[0][1], minuend.ptr, keep[1][1], None if addend is None else addend.ptr,
                                         keep[2][1], out.ptr, keep[3][1], keep[4][1], len(mod_ids), pk))

    def _fused_desc(self, src, minuend, out, mod_ids, k, mix=None, mix_k=None, addend=None, addend_k=None, in_limbs=None, mix_limbs=None,
                    minuend_limbs=None, addend_limbs=None, out_limbs=None, conv=None, addend_galois=None):
        """(hm_ntt_fused_desc, what it points to: keep alive until the call has returned)"""
        keep = [_u32(x) for x in (in_limbs, mix_limbs, minuend_limbs, addend_limbs, out_limbs, mod_ids)]
        ks = [_u64(x) for x in (mix_k, addend_k, k)]
        kg = _u32(addend_galois)   # per limb: read the addend through the automorphism X -> X^g
        ptr = lambda v: None if v is None else v.ptr
        descs, keep2 = None, []
        if conv:
            descs = (hm_bconv_desc * len(conv))()
            for dd, (csrc, c_in_limbs, in_ids, c_out_limbs, out_ids, *pk) in zip(descs, conv):
                arrs = [_u32(c_in_limbs), _u32(in_ids), _u32(c_out_limbs), _u32(out_ids)]
                keep2.append(arrs)
                dd.in_packed = 1 if pk and pk[0] else 0
                dd.in_, dd.in_limbs, dd.in_ids, dd.n_in = csrc.ptr, arrs[0][1], arrs[1][1], len(in_ids)
                dd.out, dd.out_limbs, dd.out_ids, dd.n_out, dd.log_len = out.ptr, arrs[2][1], arrs[3][1], len(out_ids), 0
        d = hm_ntt_fused_desc(ptr(src) if src is not None else out.ptr, keep[0][1], ptr(mix), keep[1][1], ks[0][1], minuend.ptr, keep[2][1], ptr(addend), keep[3][1], ks[1][1],
                              out.ptr, keep[4][1], keep[5][1], len(mod_ids), ks[2][1], C.cast(descs, C.c_void_p) if conv else None, len(conv) if conv else 0,
                              kg[1])
        return d, (keep, ks, kg, descs, keep2)

    def ntt_mix_sub_scale(self, src, minuend, out, mod_ids, k, mix=None, mix_k=None, addend=None, addend_k=None, in_limbs=None,
                          mix_limbs=None, minuend_limbs=None, addend_limbs=None, out_limbs=None, conv=None, addend_galois=None):
        """out = (minuend - NTT(src + mix_k * mix)) * k + addend * addend_k (merged ModDown + rescale of one limb).
        conv = [(src, in_limbs, in_ids, out_limbs_of_the_fed_limb_polys, out_ids), ...]: `src` of those limb-polys is this base conversion,
        computed inside the transform's first pass (src may then be None)"""
        d, keep = self._fused_desc(src, minuend, out, mod_ids, k, mix, mix_k, addend, addend_k, in_limbs, mix_limbs, minuend_limbs, addend_limbs,
                                   out_limbs, conv, addend_galois)
        self._ck(self.L.hm_ntt_mix_sub_scale(self.h, C.byref(d)))

    def ntt_mix_sub_scale_mul(self, src, minuend, minuend_b, out, mod_ids, k, minuend_b_limbs=None, mix=None, mix_k=None, addend=None, addend_k=None,
                              in_limbs=None, mix_limbs=None, minuend_limbs=None, addend_limbs=None, out_limbs=None):
        """out = (minuend (.) minuend_b - NTT(src + mix_k * mix)) * k + addend * addend_k: ntt_mix_sub_scale with a product minuend formed while the
        epilogue loads (hm_ntt_mix_sub_scale_mul); NO_LIMB in minuend_b_limbs = a plain minuend for that limb-poly"""
        d, keep = self._fused_desc(src, minuend, out, mod_ids, k, mix, mix_k, addend, addend_k, in_limbs, mix_limbs, minuend_limbs, addend_limbs, out_limbs)
        kb = _u32(minuend_b_limbs)
        m = hm_ntt_fused_mul_desc(d, minuend_b.ptr, kb[1])
        self._ck(self.L.hm_ntt_mix_sub_scale_mul(self.h, C.byref(m)))

    def tensor(self, a, b, c, d, o0, o1, o2, mod_ids, limbs=None):
        ls = limbs or [None] * 7
        keep = [_u32(x) for x in ls] + [_u32(mod_ids)]
        self._ck(self.L.hm_tensor(self.h, a.ptr, keep[0][1], b.ptr, keep[1][1], c.ptr, keep[2][1], d.ptr, keep[3][1], o0.ptr, keep[4][1],
                                  o1.ptr, keep[5][1], o2.ptr, keep[6][1], keep[7][1], len(mod_ids)))

    def tensor_dot(self, a, b, c, d, o0, o1, o2, mod_ids, n_terms, limbs=None):
        """o0 = sum_t a_t * b_t, o1 = sum_t (a_t * d_t + c_t * b_t), o2 = sum_t c_t * d_t over n_terms pairs per entry (hm_tensor_dot).  limbs: the
        seven limb lists in argument order (None: the identity), a .. d [n][n_terms], o0 .. o2 [n]; buffers: anything with a device address `.ptr`"""
        ls = limbs or [None] * 7
        keep = [_u32(x) for x in ls] + [_u32(mod_ids)]
        self._ck(self.L.hm_tensor_dot(self.h, a.ptr, keep[0][1], b.ptr, keep[1][1], c.ptr, keep[2][1], d.ptr, keep[3][1], o0.ptr, keep[4][1],
                                      o1.ptr, keep[5][1], o2.ptr, keep[6][1], keep[7][1], len(mod_ids), int(n_terms)))

    def tensor_square(self, a, c, o0, o1, o2, mod_ids, scale=None, addend=None, limbs=None):
        """o0 = s * a * a + k, o1 = 2 * s * a * c, o2 = s * c * c per entry, s = scale[i] (None: 1) and k = addend[i] (None: 0) residues of the
        entry's modulus (hm_tensor_square).  limbs: the five limb lists in argument order (None: the identity), [n] each; buffers: anything with
        a device address `.ptr`"""
        ls = limbs or [None] * 5
        keep = [_u32(x) for x in ls] + [_u32(mod_ids)]
        ks, ka = _u64(scale), _u64(addend)
        self._ck(self.L.hm_tensor_square(self.h, a.ptr, keep[0][1], c.ptr, keep[1][1], o0.ptr, keep[2][1], o1.ptr, keep[3][1], o2.ptr, keep[4][1],
                                         keep[5][1], len(mod_ids), ks[1], ka[1]))

    def lincomb(self, src, in_limbs, out, out_limbs, mod_ids, n_terms, scale, addend=None):
        """out[i] = sum_t scale[i][t] * src[in_limbs[i][t]] + addend[i] per entry (hm_lincomb): in_limbs and scale are row-major [n][n_terms]
        (flat), out_limbs and mod_ids [n] (a limb list None: the identity), scale and addend residues of the entry's modulus (addend None: 0);
        buffers: anything with a device address `.ptr`"""
        keep = [_u32(in_limbs), _u32(out_limbs), _u32(mod_ids)]
        ks, ka = _u64(scale), _u64(addend)
        self._ck(self.L.hm_lincomb(self.h, src.ptr, keep[0][1], out.ptr, keep[1][1], keep[2][1], len(mod_ids), int(n_terms), ks[1], ka[1]))

    def lincomb_multi(self, src, in_limbs, out, out_limbs, mod_ids, n_terms, n_out, scale, addend=None):
        """out[out_limbs[i][m]] = sum_t scale[i][m][t] * src[in_limbs[i][t]] + addend[i][m] per entry and output (hm_lincomb_multi): in_limbs is
        row-major [n][n_terms], out_limbs and addend [n][n_out], scale [n][n_out][n_terms] (all flat), mod_ids [n] (a limb list None: the
        identity), scale and addend residues of the entry's modulus (addend None: 0); buffers: anything with a device address `.ptr`"""
        keep = [_u32(in_limbs), _u32(out_limbs), _u32(mod_ids)]
        ks, ka = _u64(scale), _u64(addend)
        self._ck(self.L.hm_lincomb_multi(self.h, src.ptr, keep[0][1], out.ptr, keep[1][1], keep[2][1], len(mod_ids), int(n_terms), int(n_out),
                                         ks[1], ka[1]))

    def tensor_muladd(self, a, b, c, d, x, o0, o1, o2, mod_ids, n_addends=0, x0_limbs=None, x1_limbs=None, scale=None, add_scale=None, addend=None,
                      limbs=None):
        """o0 = s * a * b + sum_t u_t * x_t + k, o1 = s * (a * d + c * b) + sum_t u_t * y_t, o2 = s * c * d per entry (hm_tensor_muladd): s =
        scale[i] (None: 1), u_t = add_scale[i][t], k = addend[i] (None: 0), residues of the entry's modulus; x_t / y_t = the limb-polys
        x0_limbs[i][t] / x1_limbs[i][t] of the buffer x (row-major [n][n_addends], flat; x and the three lists may be None at n_addends = 0).
        limbs: the seven limb lists of a, b, c, d, o0, o1, o2 (None: the identity), [n] each; buffers: anything with a device address `.ptr`"""
        ls = limbs or [None] * 7
        keep = [_u32(v) for v in ls] + [_u32(x0_limbs), _u32(x1_limbs), _u32(mod_ids)]
        ks, ku, ka = _u64(scale), _u64(add_scale), _u64(addend)
        self._ck(self.L.hm_tensor_muladd(self.h, a.ptr, keep[0][1], b.ptr, keep[1][1], c.ptr, keep[2][1], d.ptr, keep[3][1],
                                         x.ptr if x is not None else None, keep[7][1], keep[8][1], o0.ptr, keep[4][1], o1.ptr, keep[5][1],
                                         o2.ptr, keep[6][1], keep[9][1], len(mod_ids), int(n_addends), ks[1], ku[1], ka[1]))

    def reim_split(self, x, y, o_re, o_im, mod_ids, limbs=None):
        """o_re = x + y, o_im = U * (x - y) per entry, U the evaluation form of -X^(N/2) under the entry's modulus, derived by the back-end from
        its own roots (hm_reim_split).  limbs: the four limb lists of x, y, o_re, o_im (None: the identity), [n] each; buffers: anything with
        a device address `.ptr`"""
        ls = limbs or [None] * 4
        keep = [_u32(v) for v in ls] + [_u32(mod_ids)]
        self._ck(self.L.hm_reim_split(self.h, x.ptr, keep[0][1], y.ptr, keep[1][1], o_re.ptr, keep[2][1], o_im.ptr, keep[3][1], keep[4][1],
                                      len(mod_ids)))

    def clincomb(self, src, in_limbs, out, out_limbs, mod_ids, n_terms, scale_re, scale_im=None, addend_re=None, addend_im=None):
        """out[i] = sum_t (scale_re[i][t] + scale_im[i][t] * X^(N/2)) * src[in_limbs[i][t]] + addend_re[i] + addend_im[i] * X^(N/2) per entry
        (hm_clincomb): in_limbs and the scalars are row-major [n][n_terms] (flat), out_limbs and mod_ids [n] (a limb list None: the identity), all
        constants residues of the entry's modulus (scale_im / addend_re / addend_im None: 0); the back-end derives X^(N/2) from its own roots;
        buffers: anything with a device address `.ptr`"""
        keep = [_u32(in_limbs), _u32(out_limbs), _u32(mod_ids)]
        ks = [_u64(v) for v in (scale_re, scale_im, addend_re, addend_im)]
        self._ck(self.L.hm_clincomb(self.h, src.ptr, keep[0][1], out.ptr, keep[1][1], keep[2][1], len(mod_ids), int(n_terms), ks[0][1], ks[1][1],
                                    ks[2][1], ks[3][1]))

    def plincomb(self, p, p_limbs, x, x0_limbs, x1_limbs, out, o0_limbs, o1_limbs, mod_ids, n_terms, addend=None, addend_limbs=None):
        """out[o0_limbs[i]] = sum_t p[p_limbs[i][t]] * x[x0_limbs[i][t]] + addend[addend_limbs[i]], out[o1_limbs[i]] = sum_t p[p_limbs[i][t]] *
        x[x1_limbs[i][t]] per entry, coefficient by coefficient (hm_plincomb): the term lists are row-major [n][n_terms] (flat), the output and
        addend lists and mod_ids [n] (a limb list None: the identity); addend None: no addend; buffers: anything with a device address `.ptr`"""
        keep = [_u32(v) for v in (p_limbs, x0_limbs, x1_limbs, addend_limbs, o0_limbs, o1_limbs, mod_ids)]
        self._ck(self.L.hm_plincomb(self.h, p.ptr, keep[0][1], x.ptr, keep[1][1], keep[2][1], None if addend is None else addend.ptr, keep[3][1],
                                    out.ptr, keep[4][1], keep[5][1], keep[6][1], len(mod_ids), int(n_terms)))

    def tensor_dotadd(self, a, b, c, d, x, o0, o1, o2, mod_ids, n_terms, n_addends=0, x0_limbs=None, x1_limbs=None, scale=None, add_scale=None,
                      addend=None, limbs=None):
        """o0 = sum_t s_t * a_t * b_t + sum_r u_r * x_r + k, o1 = sum_t s_t * (a_t * d_t + c_t * b_t) + sum_r u_r * y_r, o2 = sum_t s_t * c_t *
        d_t per entry (hm_tensor_dotadd): s_t = scale[i][t] (None: 1), u_r = add_scale[i][r], k = addend[i] (None: 0), residues of the entry's
        modulus; x_r / y_r = the limb-polys x0_limbs[i][r] / x1_limbs[i][r] of the buffer x (row-major [n][n_addends], flat; x and the three
        lists may be None at n_addends = 0).  limbs: the seven limb lists of a, b, c, d ([n][n_terms], flat) and o0, o1, o2 ([n]) (None: the
        identity); buffers: anything with a device address `.ptr`"""
        ls = limbs or [None] * 7
        keep = [_u32(v) for v in ls] + [_u32(x0_limbs), _u32(x1_limbs), _u32(mod_ids)]
        ks, ku, ka = _u64(scale), _u64(add_scale), _u64(addend)
        self._ck(self.L.hm_tensor_dotadd(self.h, a.ptr, keep[0][1], b.ptr, keep[1][1], c.ptr, keep[2][1], d.ptr, keep[3][1],
                                         x.ptr if x is not None else None, keep[7][1], keep[8][1], o0.ptr, keep[4][1], o1.ptr, keep[5][1],
                                         o2.ptr, keep[6][1], keep[9][1], len(mod_ids), int(n_terms), int(n_addends), ks[1], ku[1], ka[1]))

    def inner_product(self, x, x_limbs, y, y_limbs, out, out_limbs, mod_ids, n_terms, n_out, x_galois=0):
        keep = [_u32(v) for v in (x_limbs, y_limbs, out_limbs, mod_ids)]
        if x_galois:   # the x operands through the automorphism X -> X^g (hm_inner_product_ex)
            d = hm_ip_desc(x.ptr, keep[0][1], y.ptr, keep[1][1], out.ptr, keep[2][1], keep[3][1], len(mod_ids), n_terms, n_out, int(x_galois))
            self._ck(self.L.hm_inner_product_ex(self.h, C.byref(d)))
            return
        self._ck(self.L.hm_inner_product(self.h, x.ptr, keep[0][1], y.ptr, keep[1][1], out.ptr, keep[2][1], keep[3][1], len(mod_ids),
                                         n_terms, n_out))

    def inner_product_hoisted(self, x, x_limbs, y, y_limbs, out, out_limbs, mod_ids, n_terms, galois):
        """out[r][i][k] = sum_j automorph_{galois[r]}(x[i][j]) * y[r][i][k][j], k < 2: the key products of len(galois) rotations of one
        ciphertext from its unrotated digits, the digits read once (hm_inner_product_hoisted).  Limb lists: x_limbs [n][n_terms],
        y_limbs [r][n][2][n_terms], out_limbs [r][n][2]; x / y / out: anything with a device address `.ptr`"""
        keep = [_u32(v) for v in (x_limbs, y_limbs, out_limbs, mod_ids, galois)]
        d = hm_ip_hoisted_desc(x.ptr, keep[0][1], y.ptr, keep[1][1], out.ptr, keep[2][1], keep[3][1], len(mod_ids), n_terms, len(galois), keep[4][1])
        self._ck(self.L.hm_inner_product_hoisted(self.h, C.byref(d)))

    def inner_product_lintrans(self, x, x_limbs, y, y_limbs, pt, pt_limbs, out, out_limbs, mod_ids, n_terms, galois,
                               addend=None, addend_limbs=None, addend_out=None, addend_out_limbs=None):
        """out[i][k] = sum_r pt[r][i] * sum_j automorph_{galois[r]}(x[i][j]) * y[r][i][k][j], k < 2, and for the entries with an addend source
        (addend_limbs[i] != NO_LIMB) addend_out[i] = sum_r pt[r][i] * automorph_{galois[r]}(addend[i]) (hm_inner_product_lintrans).  Limb lists:
        x_limbs [n][n_terms], y_limbs [r][n][2][n_terms], pt_limbs [r][n], out_limbs [n][2], addend_limbs / addend_out_limbs [n]"""
        keep = [_u32(v) for v in (x_limbs, y_limbs, pt_limbs, addend_limbs, out_limbs, addend_out_limbs, mod_ids, galois)]
        ptr = lambda v: None if v is None else v.ptr
        d = hm_ip_lintrans_desc(x.ptr, keep[0][1], y.ptr, keep[1][1], pt.ptr, keep[2][1], ptr(addend), keep[3][1], out.ptr, keep[4][1],
                                ptr(addend_out), keep[5][1], keep[6][1], len(mod_ids), n_terms, len(galois), keep[7][1])
        self._ck(self.L.hm_inner_product_lintrans(self.h, C.byref(d)))

    def inner_product_lintrans_multi(self, x, x_limbs, y, y_limbs, pt, pt_limbs, out, out_limbs, mod_ids, n_terms, galois, n_out,
                                     addend=None, addend_limbs=None, addend_out=None, addend_out_limbs=None):
        """n_out weighted sums of the same hoisted key products: out[m][i][k] = sum_r pt[m][r][i] * t[r][i][k] with t as inner_product_lintrans
        forms it, once per rotation, and addend_out[m][i] = sum_r pt[m][r][i] * automorph_{galois[r]}(addend[i]) (hm_inner_product_lintrans_multi).
        Limb lists: x_limbs [n][n_terms], y_limbs [r][n][2][n_terms], pt_limbs [m][r][n], out_limbs [m][n][2], addend_limbs [n],
        addend_out_limbs [m][n]"""
        keep = [_u32(v) for v in (x_limbs, y_limbs, pt_limbs, addend_limbs, out_limbs, addend_out_limbs, mod_ids, galois)]
        ptr = lambda v: None if v is None else v.ptr
        d = hm_ip_lintrans_multi_desc(x.ptr, keep[0][1], y.ptr, keep[1][1], pt.ptr, keep[2][1], ptr(addend), keep[3][1], out.ptr, keep[4][1],
                                      ptr(addend_out), keep[5][1], keep[6][1], len(mod_ids), n_terms, len(galois), n_out, keep[7][1])
        self._ck(self.L.hm_inner_product_lintrans_multi(self.h, C.byref(d)))

    def inner_product_lintrans_id(self, x, x_limbs, y, y_limbs, pt, pt_limbs, out, out_limbs, mod_ids, n_terms, galois, n_out,
                                  addend, addend_limbs, addend_out, addend_out_limbs, id_pt_limbs, addend1, addend1_limbs, addend1_out, addend1_out_limbs):
        """inner_product_lintrans_multi with the identity step (hm_inner_product_lintrans_id): on the entries with an addend source,
        addend_out[m][i] += pt[id_pt_limbs[m][i]] * addend[i] and addend1_out[m][i] = pt[id_pt_limbs[m][i]] * addend1[i], both sources read
        unrotated.  Further limb lists: id_pt_limbs [m][n] (limbs of pt), addend1_limbs [n] (NO_LIMB exactly where addend_limbs is),
        addend1_out_limbs [m][n].  Any of the identity arguments may be None: the call is then refused by the library"""
        keep = [_u32(v) for v in (x_limbs, y_limbs, pt_limbs, addend_limbs, out_limbs, addend_out_limbs, mod_ids, galois, id_pt_limbs, addend1_limbs,
                                  addend1_out_limbs)]
        ptr = lambda v: None if v is None else v.ptr
        sums = hm_ip_lintrans_multi_desc(x.ptr, keep[0][1], y.ptr, keep[1][1], pt.ptr, keep[2][1], ptr(addend), keep[3][1], out.ptr, keep[4][1],
                                         ptr(addend_out), keep[5][1], keep[6][1], len(mod_ids), n_terms, len(galois), n_out, keep[7][1])
        d = hm_ip_lintrans_id_desc(sums, keep[8][1], ptr(addend1), keep[9][1], ptr(addend1_out), keep[10][1])
        self._ck(self.L.hm_inner_product_lintrans_id(self.h, C.byref(d)))

    def inner_product_rotsum(self, x, x_limbs, y, y_limbs, out, out_limbs, mod_ids, n_terms, galois,
                             addend=None, addend_limbs=None, addend_out=None, addend_out_limbs=None):
        """out[i][k] = sum_c sum_j automorph_{galois[c]}(x[c][i][j]) * y[c][i][k][j], k < 2, and for the entries with addend sources
        (addend_limbs[c][i] != NO_LIMB) addend_out[i] = sum_c automorph_{galois[c]}(addend[c][i]) (hm_inner_product_rotsum).  Limb lists:
        x_limbs [c][n][n_terms], y_limbs [c][n][2][n_terms], out_limbs [n][2], addend_limbs [c][n], addend_out_limbs [n]"""
        keep = [_u32(v) for v in (x_limbs, y_limbs, addend_limbs, out_limbs, addend_out_limbs, mod_ids, galois)]
        ptr = lambda v: None if v is None else v.ptr
        d = hm_ip_rotsum_desc(x.ptr, keep[0][1], y.ptr, keep[1][1], ptr(addend), keep[2][1], out.ptr, keep[3][1],
                              ptr(addend_out), keep[4][1], keep[5][1], len(mod_ids), n_terms, len(galois), keep[6][1])
        self._ck(self.L.hm_inner_product_rotsum(self.h, C.byref(d)))

    def inner_product_rotsum_init(self, x, x_limbs, y, y_limbs, out, out_limbs, mod_ids, n_terms, galois, init, init_limbs,
                                  addend=None, addend_limbs=None, addend_out=None, addend_out_limbs=None, addend_init_limbs=None):
        """inner_product_rotsum whose sums start from init[i][k] (limb list [n][2]) and, on the entries with addend sources, from
        addend[addend_init_limbs[i]] instead of zero (hm_inner_product_rotsum_init)"""
        keep = [_u32(v) for v in (x_limbs, y_limbs, addend_limbs, out_limbs, addend_out_limbs, mod_ids, galois, init_limbs, addend_init_limbs)]
        ptr = lambda v: None if v is None else v.ptr
        s = hm_ip_rotsum_desc(x.ptr, keep[0][1], y.ptr, keep[1][1], ptr(addend), keep[2][1], out.ptr, keep[3][1],
                              ptr(addend_out), keep[4][1], keep[5][1], len(mod_ids), n_terms, len(galois), keep[6][1])
        d = hm_ip_rotsum_init_desc(s, ptr(init), keep[7][1], keep[8][1])
        self._ck(self.L.hm_inner_product_rotsum_init(self.h, C.byref(d)))

    def ntt_second_pass(self, buf, mod_ids, inverse=False, limbs=None, scale=None):
        """the last pass of transforms whose first pass another call has already run into `buf` (in place)"""
        k1, pl = _u32(limbs)
        k2, pm = _u32(mod_ids)
        k3, ps = _u64(scale)
        self._ck(self.L.hm_ntt_second_pass(self.h, buf.ptr, pl, pm, len(mod_ids), 1 if inverse else 0, ps))

    def ntt_inner_product(self, x, x_limbs, x_is_coeff, hand, hand_limbs, y, y_limbs, out, out_limbs, mod_ids, n_terms, n_out, conv=None, out_inverse=None,
                          x_galois=0):
        """out[i][k] = sum_j (NTT(x[i][j]) if x_is_coeff[i][j] else x[i][j]) * y[i][k][j]: the HPIP unit as a fused NTT-epilogue x key MAC.
        conv = [(src, in_limbs, in_ids, hand_out_limbs, out_ids), ...]: the transformed digits are these base conversions, computed inside
        the transforms' first pass (their outputs are hand-off limbs of `hand`); x_galois = g: the evaluation-form digits are read through X -> X^g"""
        keep = [_u32(v) for v in (x_limbs, hand_limbs, y_limbs, out_limbs, mod_ids)]
        flags = np.ascontiguousarray(np.asarray(x_is_coeff, dtype=np.uint8))
        descs, keep2 = None, []
        if conv:
            descs = (hm_bconv_desc * len(conv))()
            for dd, (src, in_limbs, in_ids, out_limbs_, out_ids, *pk) in zip(descs, conv):
                arrs = [_u32(in_limbs), _u32(in_ids), _u32(out_limbs_), _u32(out_ids)]
                keep2.append(arrs)
                dd.in_packed = 1 if pk and pk[0] else 0
                dd.in_, dd.in_limbs, dd.in_ids, dd.n_in = src.ptr, arrs[0][1], arrs[1][1], len(in_ids)
                dd.out, dd.out_limbs, dd.out_ids, dd.n_out, dd.log_len = hand.ptr, arrs[2][1], arrs[3][1], len(out_ids), 0
        inv = None if out_inverse is None else np.ascontiguousarray(np.asarray(out_inverse, dtype=np.uint8))
        d = hm_ntt_ip_desc(x.ptr, keep[0][1], flags.ctypes.data_as(C.c_void_p), None if hand is None else hand.ptr, keep[1][1], y.ptr, keep[2][1],
                           out.ptr, keep[3][1], keep[4][1], len(mod_ids), n_terms, n_out,
                           C.cast(descs, C.c_void_p) if conv else None, len(conv) if conv else 0,
                           None if inv is None else inv.ctypes.data_as(C.c_void_p), int(x_galois))
        self._ck(self.L.hm_ntt_inner_product(self.h, C.byref(d)))

    # ---- slot vectors <-> plaintexts (hm_encode / hm_decode)
    def largest_modulus(self):
        return max(range(len(self.moduli)), key=lambda m: self.moduli[m])

    def encode(self, z, scale, mod_ids, src_mod=None, n_vec=None, work=None, work_limbs=None, out=None, out_limbs=None):
        """The plaintexts of slot vectors z at scale `scale` on the moduli mod_ids (hm_encode).
        z on the host: complex128, [n] or [n_vec][n] with n = N / 2; returns uint64 [n_vec][len(mod_ids)][N] in evaluation form, or, with
        mod_ids empty, the coefficient-form residues of the source modulus, [n_vec][N].
        z on the device (a DeviceBuf, or anything with data_ptr(): a contiguous complex128 torch tensor; whoever filled it has synchronised):
        n_vec vectors (default: what z.numel() holds, else 1); returns the DeviceBuf that holds the result, limb-polys in the same order
        (`out`, or `work` when mod_ids is empty).  With `work` (and `out`) given the call only enqueues on the context's stream and can be
        captured; a `work` left to default is a fresh buffer freed behind the call, which synchronises and cannot happen inside a capture.
        src_mod: the modulus the coefficients are rounded into (default: the largest of the chain); work / out: buffers of the caller's, with their
        limb lists, instead of fresh ones."""
        n = self.N // 2
        mod_ids = [int(m) for m in mod_ids]
        src_mod = self.largest_modulus() if src_mod is None else int(src_mod)
        host = not _on_device(z)
        tmp = []
        if host:
            a = np.ascontiguousarray(np.asarray(z, dtype=np.complex128)).reshape(-1, n)
            n_vec = a.shape[0]
            zbuf = self.alloc(max(1, n_vec))
            tmp.append(zbuf)
            if n_vec:
                self._ck(self.L.hm_memcpy_h2d(self.h, zbuf.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes))
            zptr = zbuf.ptr
        else:
            if n_vec is None:
                n_vec = z.numel() // n if hasattr(z, "numel") else 1
            zptr = _dev_ptr(z)
        if work is None:
            work = self.alloc(max(1, n_vec))
            if host or mod_ids:
                tmp.append(work)
        if out is None and mod_ids:
            out = self.alloc(max(1, n_vec * len(mod_ids)))
            if host:
                tmp.append(out)
        k1, pw = _u32(work_limbs)
        k2, po = _u32(out_limbs)
        k3, pm = _u32(mod_ids)
        try:
            self._ck(self.L.hm_encode(self.h, zptr, n_vec, float(scale), _dev_ptr(work), pw, src_mod, None if out is None else _dev_ptr(out), po, pm,
                                      len(mod_ids)))
            if not host:
                return out if mod_ids else work
            res, rows = (out, n_vec * len(mod_ids)) if mod_ids else (work, n_vec)
            limbs = (out_limbs if mod_ids else work_limbs)
            got = np.empty((rows, self.N), dtype=np.uint64)
            for r in range(rows):
                self._ck(self.L.hm_memcpy_d2h(self.h, got[r].ctypes.data_as(C.c_void_p), _dev_ptr(res) + 8 * self.N * (r if limbs is None else int(limbs[r])),
                                              8 * self.N))
            return got.reshape(n_vec, len(mod_ids), self.N) if mod_ids else got
        finally:
            for b in tmp:
                b.free()

    def decode(self, buf, limbs, mod_id, scale, work=None, work_limbs=None, out=None):
        """The slots of evaluation-form limb-polys modulo q_(mod_id) at scale `scale` (hm_decode), one vector per entry of `limbs` (None: the rows
        of buf in order).
        buf on the host: uint64 [rows][N]; returns complex128 [n_vec][N / 2].
        buf on the device (a DeviceBuf or anything with data_ptr()): `limbs` must be given; returns `out` (anything on the device with room for
        n_vec x N / 2 complex128, 16-byte aligned; default: a fresh DeviceBuf of n_vec limb-polys, vector v in limb-poly v as (re, im) doubles).
        With `work` given the call only enqueues and can be captured; a default `work` is freed behind the call, which synchronises."""
        n = self.N // 2
        host = not _on_device(buf)
        tmp = []
        if host:
            a = np.ascontiguousarray(buf, dtype=np.uint64).reshape(-1, self.N)
            n_vec = a.shape[0] if limbs is None else len(limbs)
            src = self.from_host(a) if a.shape[0] else self.alloc(1)
            tmp.append(src)
        else:
            n_vec = len(limbs)
            src = buf
        if work is None:
            work = self.alloc(max(1, n_vec))
            tmp.append(work)
        if out is None:
            out = self.alloc(max(1, n_vec))
            if host:
                tmp.append(out)
        k1, pi = _u32(limbs)
        k2, pw = _u32(work_limbs)
        try:
            self._ck(self.L.hm_decode(self.h, _dev_ptr(src), pi, int(mod_id), float(scale), _dev_ptr(work), pw, _dev_ptr(out), n_vec))
            if not host:
                return out
            got = np.empty((n_vec, n), dtype=np.complex128)
            if n_vec:
                self._ck(self.L.hm_memcpy_d2h(self.h, got.ctypes.data_as(C.c_void_p), _dev_ptr(out), got.nbytes))
            return got
        finally:
            for b in tmp:
                b.free()

    def automorph(self, src, dst, n, galois, in_limbs=None, out_limbs=None):
        k1, pi = _u32(in_limbs)
        k2, po = _u32(out_limbs)
        self._ck(self.L.hm_automorph(self.h, src.ptr, pi, dst.ptr, po, n, galois))

    def ewe(self, op, out, mod_ids, a=None, b=None, c=None, d=None, la=None, lb=None, lc=None, ld=None, lo=None, k=None):
        keep = [_u32(x) for x in (la, lb, lc, ld, lo, mod_ids)]
        kk, pk = _u64(k)
        ptr = lambda x: None if x is None else x.ptr
        self._ck(self.L.hm_ewe(self.h, op, ptr(a), keep[0][1], ptr(b), keep[1][1], ptr(c), keep[2][1], ptr(d), keep[3][1],
                               out.ptr, keep[4][1], keep[5][1], len(mod_ids), pk))

    def bconv(self, src, in_ids, dst, out_ids, in_limbs=None, out_limbs=None):
        k1, pil = _u32(in_limbs)
        k2, pii = _u32(in_ids)
        k3, pol = _u32(out_limbs)
        k4, poi = _u32(out_ids)
        self._ck(self.L.hm_bconv(self.h, src.ptr, pil, pii, len(in_ids), dst.ptr, pol, poi, len(out_ids)))

    @staticmethod
    def _bconv_descs(probs, log_len=0):
        keep, descs = [], (hm_bconv_desc * len(probs))()
        for d, (src, in_limbs, in_ids, dst, out_limbs, out_ids, *pk) in zip(descs, probs):
            arrs = [_u32(in_limbs), _u32(in_ids), _u32(out_limbs), _u32(out_ids)]
            keep.append(arrs)
            d.in_packed = 1 if pk and pk[0] else 0
            d.in_, d.in_limbs, d.in_ids, d.n_in = src.ptr, arrs[0][1], arrs[1][1], len(in_ids)
            d.out, d.out_limbs, d.out_ids, d.n_out, d.log_len = dst.ptr, arrs[2][1], arrs[3][1], len(out_ids), log_len
        return keep, descs

    def bconv_batch(self, probs, log_len=0):
        """several conversions in one launch: probs = [(src, in_limbs, in_ids, dst, out_limbs, out_ids[, in_packed]), ...]"""
        keep, descs = self._bconv_descs(probs, log_len)
        self._ck(self.L.hm_bconv_batch(self.h, descs, len(probs)))

    def bconv_col(self, probs, tile0=0, n_tiles=0):
        """conversion + first pass of the forward transform of every output, on the column tiles [tile0, tile0 + n_tiles) (n_tiles = 0: all):
        the same `probs` tuples as bconv_batch; every dst must be the one hand-off buffer of the call (hm_bconv_col)"""
        keep, descs = self._bconv_descs(probs)
        self._ck(self.L.hm_bconv_col(self.h, descs, len(probs), int(tile0), int(n_tiles)))

    def bconv_consts(self, in_ids, out_ids):
        k1, pii = _u32(in_ids)
        k2, poi = _u32(out_ids)
        qh = np.empty(len(in_ids), dtype=np.uint64)
        tb = np.empty((len(in_ids), max(1, len(out_ids))), dtype=np.uint64)
        self._ck(self.L.hm_bconv_consts(self.h, pii, len(in_ids), poi, len(out_ids), qh.ctypes.data_as(C.c_void_p),
                                        tb.ctypes.data_as(C.c_void_p)))
        return qh, tb[:, :len(out_ids)]

    # ---- several ranks: the exchanges around the base conversions (buffers: anything with a device address `.ptr`)
    def comm_init_external(self, rank, world, fn):
        """collective: every rank of the communicator calls it at the same time.  fn: an hm_exchange_fn (homulator_amd.dist.EXCHANGE_FN), kept
        alive by this context"""
        self._exchange_fn = fn
        self._ck(self.L.hm_comm_init_external(self.h, int(rank), int(world), C.cast(fn, C.c_void_p), None))

    def limbs_to_slices(self, buf, limbs, owners, slices):
        k1, pl = _u32(limbs)
        k2, po = _u32(owners)
        self._ck(self.L.hm_limbs_to_slices(self.h, buf.ptr, pl, po, len(owners), slices.ptr))

    def slices_to_limbs(self, slices, buf, limbs, owners):
        k1, pl = _u32(limbs)
        k2, po = _u32(owners)
        self._ck(self.L.hm_slices_to_limbs(self.h, slices.ptr, buf.ptr, pl, po, len(owners)))

    def limbs_to_colslices(self, buf, limbs, owners, slices):
        k1, pl = _u32(limbs)
        k2, po = _u32(owners)
        self._ck(self.L.hm_limbs_to_colslices(self.h, buf.ptr, pl, po, len(owners), slices.ptr))

    def colslices_to_limbs(self, slices, buf, limbs, owners):
        k1, pl = _u32(limbs)
        k2, po = _u32(owners)
        self._ck(self.L.hm_colslices_to_limbs(self.h, slices.ptr, buf.ptr, pl, po, len(owners)))

    def replicate_limbs(self, buf, limbs, owners):
        k1, pl = _u32(limbs)
        k2, po = _u32(owners)
        self._ck(self.L.hm_replicate_limbs(self.h, buf.ptr, pl, po, len(owners)))

    def fill_uniform(self, dst, mod_ids, seed, out_limbs=None):
        k1, pol = _u32(out_limbs)
        k2, pm = _u32(mod_ids)
        self._ck(self.L.hm_fill_uniform(self.h, dst.ptr, pol, pm, len(mod_ids), int(seed) & (2 ** 64 - 1)))

    def set_option(self, name, value):
        self._ck(self.L.hm_set_option(self.h, name.encode(), int(value)))

    def counter(self, name):
        v = C.c_uint64()
        self._ck(self.L.hm_get_counter(self.h, name.encode(), C.byref(v)))
        return v.value

    def timer_start(self):
        self._ck(self.L.hm_timer_start(self.h))

    def timer_stop(self):
        ns = C.c_uint64()
        self._ck(self.L.hm_timer_stop(self.h, C.byref(ns)))
        return ns.value
