"""ctypes binding of libidmvton_hip.so -- a field-for-field mirror of include/idmvton_hip.h.

The mirror is verified at load time against `idmvton_sizeof()` exported by the library, so a drift between this file
and the header fails loudly instead of corrupting kernel arguments.
"""
import ctypes as C
import functools
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IDMVTON_HIP_LIB") or os.path.join(_HERE, "libidmvton_hip.so")   # override: A/B of library builds

F16, BF16, F32, F8E4M3 = 0, 1, 2, 3
EPI_NONE, EPI_GEGLU, EPI_GELU, EPI_QUICKGELU, EPI_XATTN = 0, 1, 2, 3, 4
ATTN_SELF, ATTN_CROSS = 0, 1
IO_RES_F32, IO_OUT_F32, IO_BIAS_F32, IO_OUT_F8 = 1, 2, 4, 8
GN_X_F32, GN_Y_SPLIT, GN_AFFINE_F32 = 1, 2, 4
LAYOUT_SPLIT, LAYOUT_NHWC_F32 = 1, 2
SPLIT_ACT, SPLIT_W3, SPLIT_W3T = 0, 1, 2
KVS_WIDEN_E4M3, KVS_COPY = 0, 1
MAX_SEG = 24
ABI_VERSION = 9

i32, u32, f32, vp = C.c_int32, C.c_uint32, C.c_float, C.c_void_p


class Seg(C.Structure):
    _fields_ = [("ptr", vp), ("bytes", u32), ("pitch", i32), ("coff", i32), ("len", i32), ("dy", i32), ("dx", i32)]


class XAttn(C.Structure):
    _fields_ = [("nseg", i32), ("k", vp * 2), ("ldk", i32 * 2), ("k_rows", i32 * 2), ("vt", vp * 2), ("ldvt", i32 * 2), ("nk", i32 * 2),
                ("tokens", i32), ("ip_scale", f32)]


class GemmConvArgs(C.Structure):
    _fields_ = [("dtype", i32), ("w", vp), ("N", i32), ("Ktot", i32), ("nseg", i32), ("seg", Seg * MAX_SEG),
                ("M", i32), ("Ho", i32), ("Wo", i32), ("Hi", i32), ("Wi", i32), ("stride", i32), ("ups", i32),
                ("out", vp), ("ldo", i32), ("bias", vp), ("rowbias", vp), ("rowbias_ld", i32),
                ("rows_per_group", i32), ("res", vp), ("ldr", i32), ("mode", i32), ("vt", vp), ("vt_n0", i32),
                ("vt_tokens", i32), ("tile_hint", i32), ("vt_perm", i32), ("io_flags", i32), ("xattn", C.POINTER(XAttn)),
                ("colscale_n", i32), ("colscale", f32), ("f8_out_scale", f32), ("f8_vt_scale", f32)]


class AttnArgs(C.Structure):
    _fields_ = [("dtype", i32), ("mode", i32), ("B", i32), ("heads", i32), ("Nq", i32), ("q", vp), ("ldq", i32),
                ("out", vp), ("ldo", i32), ("nseg", i32), ("k", vp * 2), ("ldk", i32 * 2), ("vt", vp * 2),
                ("ldvt", i32 * 2), ("nk", i32 * 2), ("k_rows", i32 * 2), ("seg_b0", i32 * 2), ("ip_scale", f32), ("tune", i32), ("q_prescaled", i32)]


class LayerNormArgs(C.Structure):
    _fields_ = [("dtype", i32), ("rows", i32), ("C", i32), ("x", vp), ("ldx", i32), ("gamma", vp), ("beta", vp),
                ("eps", f32), ("y", vp), ("ldy", i32), ("y2", vp), ("ldy2", i32), ("x_f32", i32)]


class GroupNormArgs(C.Structure):
    _fields_ = [("dtype", i32), ("B", i32), ("HW", i32), ("C", i32), ("groups", i32), ("x", vp), ("C1", i32),
                ("x2", vp), ("gamma", vp), ("beta", vp), ("eps", f32), ("silu", i32), ("y", vp), ("stats", vp), ("stats_doubles", i32),
                ("flags", i32)]


class PackInputArgs(C.Structure):
    _fields_ = [("dtype", i32), ("B", i32), ("hw", i32), ("cpad", i32), ("latents", vp), ("cond", vp), ("out", vp)]


class CfgStepArgs(C.Structure):
    _fields_ = [("dtype", i32), ("B", i32), ("hw", i32), ("ldc", i32), ("eps_nhwc", vp), ("latents", vp),
                ("noise", vp), ("coef", vp)]


class GuidedStepArgs(C.Structure):
    _fields_ = [("dtype", i32), ("B", i32), ("hw", i32), ("ldc", i32), ("branches", i32), ("work_floats", i32), ("eps_nhwc", vp),
                ("latents", vp), ("noise", vp), ("coef", vp), ("work", vp)]


class PersonStepArgs(C.Structure):                       # idmvton_guided_step_args' fields; the coef row has a third column, active[B]
    _fields_ = list(GuidedStepArgs._fields_)


class PackRowsArgs(C.Structure):                         # a row plan's TryonNet input: row r is person row_person[r] (a device table)
    _fields_ = [("dtype", i32), ("B", i32), ("R", i32), ("hw", i32), ("cpad", i32), ("latents", vp), ("cond", vp), ("out", vp),
                ("row_person", vp)]


class RowStepArgs(C.Structure):                          # the person step with eps rows looked up in the device table {urow[B], crow[B]}
    _fields_ = [("dtype", i32), ("B", i32), ("R", i32), ("hw", i32), ("ldc", i32), ("work_floats", i32), ("eps_nhwc", vp),
                ("latents", vp), ("noise", vp), ("coef", vp), ("work", vp), ("rows", vp)]


class LayoutArgs(C.Structure):
    _fields_ = [("dtype", i32), ("B", i32), ("C", i32), ("HW", i32), ("cpad", i32), ("to_nhwc", i32), ("src", vp),
                ("dst", vp), ("scale", f32), ("shift", f32), ("flags", i32)]


class VaeSampleArgs(C.Structure):
    _fields_ = [("dtype", i32), ("B", i32), ("hw", i32), ("ldm", i32), ("moments", vp), ("noise", vp), ("z", vp),
                ("scale", f32)]


class AttnSmallArgs(C.Structure):
    _fields_ = [("dtype", i32), ("B", i32), ("heads", i32), ("Lq", i32), ("Lk", i32), ("d", i32), ("q", vp), ("ldq", i32),
                ("k", vp), ("ldk", i32), ("v", vp), ("ldv", i32), ("out", vp), ("ldo", i32), ("scale", f32), ("causal", i32)]


class AttnF8Args(C.Structure):
    _fields_ = [("out_dtype", i32), ("B", i32), ("heads", i32), ("Nq", i32), ("q8", vp), ("ldq", i32), ("out", vp), ("ldo", i32),
                ("nseg", i32), ("k8", vp * 2), ("ldk", i32 * 2), ("vt8", vp * 2), ("ldvt", i32 * 2), ("nk", i32 * 2), ("k_rows", i32 * 2),
                ("seg_b0", i32 * 2), ("qk_scale_exp", i32), ("v_scale_exp", i32)]


class QuantF8Args(C.Structure):
    _fields_ = [("dtype", i32), ("mode", i32), ("rows", i32), ("cols", i32), ("src", vp), ("lds", i32), ("dst", vp), ("ldd", i32), ("scale", f32)]


class SoftmaxArgs(C.Structure):
    _fields_ = [("dtype", i32), ("rows", i32), ("n", i32), ("ld", i32), ("x", vp), ("scale", f32), ("y_split", vp), ("ldy", i32), ("n_valid", i32)]


class SplitArgs(C.Structure):
    _fields_ = [("dtype", i32), ("mode", i32), ("rows", i32), ("cols", i32), ("src", vp), ("lds", i32), ("dst", vp), ("ldd", i32)]


class KvUnpackDesc(C.Structure):
    _fields_ = [("src", vp), ("dst", vp), ("exp", vp), ("rows", i32), ("cols", i32), ("lds", i32), ("ldd", i32)]


class KvUnpackArgs(C.Structure):
    _fields_ = [("dtype", i32), ("n", i32), ("desc", vp), ("max_chunks", i32)]


class KvStreamDesc(KvUnpackDesc):                        # typedef idmvton_kv_unpack_desc idmvton_kv_stream_desc: one table builder serves both
    pass


class KvStreamArgs(C.Structure):
    _fields_ = [("dtype", i32), ("mode", i32), ("n", i32), ("workgroups", i32), ("desc", vp), ("first", vp)]


STRUCTS = {"idmvton_seg": Seg, "idmvton_gemm_conv_args": GemmConvArgs, "idmvton_attn_args": AttnArgs,
           "idmvton_layernorm_args": LayerNormArgs, "idmvton_groupnorm_args": GroupNormArgs,
           "idmvton_pack_input_args": PackInputArgs, "idmvton_cfg_step_args": CfgStepArgs,
           "idmvton_layout_args": LayoutArgs, "idmvton_vae_sample_args": VaeSampleArgs, "idmvton_softmax_args": SoftmaxArgs,
           "idmvton_attn_small_args": AttnSmallArgs, "idmvton_attn_f8_args": AttnF8Args, "idmvton_quant_f8_args": QuantF8Args,
           "idmvton_split_args": SplitArgs, "idmvton_xattn": XAttn, "idmvton_kv_unpack_desc": KvUnpackDesc,
           "idmvton_kv_unpack_args": KvUnpackArgs, "idmvton_kv_stream_desc": KvStreamDesc, "idmvton_kv_stream_args": KvStreamArgs,
           "idmvton_guided_step_args": GuidedStepArgs, "idmvton_person_step_args": PersonStepArgs,
           "idmvton_pack_rows_args": PackRowsArgs, "idmvton_row_step_args": RowStepArgs}

# every symbol include/idmvton_hip.h declares
SYMBOLS = ["idmvton_last_error", "idmvton_abi_version", "idmvton_sizeof", "idmvton_gemm_conv", "idmvton_attn_fwd",
           "idmvton_layernorm", "idmvton_groupnorm", "idmvton_pack_input", "idmvton_cfg_step", "idmvton_layout",
           "idmvton_vae_sample", "idmvton_softmax_rows", "idmvton_probe_mfma", "idmvton_groupnorm_stats_doubles",
           "idmvton_attn_small", "idmvton_rccl_unique_id", "idmvton_rccl_comm_init", "idmvton_rccl_bcast_arena",
           "idmvton_rccl_comm_destroy", "idmvton_attn_f8", "idmvton_quant_f8", "idmvton_split", "idmvton_attn_fwd_shared",
           "idmvton_attn_f8_shared", "idmvton_attn_fwd_indexed", "idmvton_attn_f8_indexed",
           "idmvton_attn_fwd_ragged", "idmvton_attn_f8_ragged", "idmvton_kv_unpack", "idmvton_kv_stream",
           "idmvton_host_device_ptr", "idmvton_kv_fill", "idmvton_kv_place", "idmvton_guided_step", "idmvton_guided_step_work_floats",
           "idmvton_pack_input_cond", "idmvton_person_step", "idmvton_pack_rows", "idmvton_row_step"]

_lib = None


class HipLibraryMissing(RuntimeError):
    pass


def lib():
    """Load libidmvton_hip.so (once).  Raises HipLibraryMissing -- never falls back to another implementation."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryMissing(f"{LIB_PATH} not built: run `make -C {os.path.join(_HERE, 'csrc')}` "
                                "(or __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    for s in SYMBOLS:
        if not hasattr(L, s):
            raise HipLibraryMissing(f"{LIB_PATH} does not export {s}")
    L.idmvton_last_error.restype = C.c_char_p
    L.idmvton_sizeof.argtypes = [C.c_char_p]
    L.idmvton_abi_version.restype = C.c_int
    v = L.idmvton_abi_version()
    if v != ABI_VERSION:                                  # semantic changes do not always move a struct size (v3 -> v5 did not): check the number too
        raise HipLibraryMissing(f"{LIB_PATH} implements C ABI version {v}, this binding needs {ABI_VERSION}: rebuild it "
                                f"(`make -C {os.path.join(_HERE, 'csrc')}`)")
    for name, st in STRUCTS.items():
        n = L.idmvton_sizeof(name.encode())
        if n != C.sizeof(st):
            raise HipLibraryMissing(f"ABI drift: sizeof({name}) is {n} in the library, {C.sizeof(st)} in ffi.py")
    for s in ("idmvton_gemm_conv", "idmvton_attn_fwd", "idmvton_layernorm", "idmvton_groupnorm",
              "idmvton_pack_input", "idmvton_cfg_step", "idmvton_layout", "idmvton_vae_sample", "idmvton_softmax_rows",
              "idmvton_attn_small", "idmvton_attn_f8", "idmvton_quant_f8", "idmvton_split", "idmvton_guided_step", "idmvton_pack_input_cond",
              "idmvton_person_step", "idmvton_pack_rows", "idmvton_row_step"):
        getattr(L, s).argtypes = [vp, vp]
        getattr(L, s).restype = C.c_int
    for s in ("idmvton_attn_fwd_shared", "idmvton_attn_f8_shared"):          # (args*, const int32_t seg_nb[2], stream)
        getattr(L, s).argtypes = [vp, C.POINTER(i32), vp]
        getattr(L, s).restype = C.c_int
    for s in ("idmvton_attn_fwd_indexed", "idmvton_attn_f8_indexed"):        # (args*, const int32_t seg_nb[2], const int32_t* const seg_index[2], stream)
        getattr(L, s).argtypes = [vp, C.POINTER(i32), C.POINTER(vp), vp]
        getattr(L, s).restype = C.c_int
    for s in ("idmvton_attn_fwd_ragged", "idmvton_attn_f8_ragged"):          # (args*, seg_nb[2], seg_index[2], const int32_t* const seg_nk[2], stream)
        getattr(L, s).argtypes = [vp, C.POINTER(i32), C.POINTER(vp), C.POINTER(vp), vp]
        getattr(L, s).restype = C.c_int
    L.idmvton_kv_unpack.argtypes = [vp, vp, vp]                               # (args*, const desc* host_desc, stream)
    L.idmvton_kv_unpack.restype = C.c_int
    for s in ("idmvton_kv_stream", "idmvton_kv_fill", "idmvton_kv_place"):    # (args*, const desc* host_desc, const int32_t* host_first, stream)
        getattr(L, s).argtypes = [vp, vp, vp, vp]
        getattr(L, s).restype = C.c_int
    L.idmvton_host_device_ptr.argtypes = [vp, C.POINTER(vp)]                  # (const void* host, void** dev)
    L.idmvton_host_device_ptr.restype = C.c_int
    L.idmvton_probe_mfma.argtypes = [C.c_int, vp, vp, vp, vp]
    L.idmvton_groupnorm_stats_doubles.argtypes = [C.c_int] * 4
    L.idmvton_groupnorm_stats_doubles.restype = C.c_int
    L.idmvton_guided_step_work_floats.argtypes = [C.c_int] * 2
    L.idmvton_guided_step_work_floats.restype = C.c_int
    L.idmvton_rccl_unique_id.argtypes = [vp]
    L.idmvton_rccl_comm_init.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.idmvton_rccl_bcast_arena.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_uint64, vp]
    L.idmvton_rccl_comm_destroy.argtypes = [vp]
    for s in ("idmvton_rccl_unique_id", "idmvton_rccl_comm_init", "idmvton_rccl_bcast_arena", "idmvton_rccl_comm_destroy"):
        getattr(L, s).restype = C.c_int
    _lib = L
    return L


def call(fn_name, args, stream):
    """Invoke an `int f(const args*, void* stream)` entry point; raise RuntimeError with the library's message."""
    L = lib()
    rc = getattr(L, fn_name)(C.byref(args), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError(f"{fn_name} failed ({rc}): {L.idmvton_last_error().decode()}")


def call_shared(fn_name, args, seg_nb, stream):
    """Invoke an `int f(const args*, const int32_t seg_nb[2], void* stream)` entry point (the shared-segment attention launches)."""
    L = lib()
    nb = (i32 * 2)(*seg_nb)
    rc = getattr(L, fn_name)(C.byref(args), nb, C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError(f"{fn_name} failed ({rc}): {L.idmvton_last_error().decode()}")


def call_indexed(fn_name, args, seg_nb, seg_index, stream):
    """Invoke an `int f(const args*, const int32_t seg_nb[2], const int32_t* const seg_index[2], void* stream)` entry point (the indexed-segment
    attention launches).  seg_index: two device addresses, 0 / None = no table for that segment."""
    L = lib()
    nb = (i32 * 2)(*seg_nb)
    ix = (vp * 2)(*[int(x) if x else None for x in seg_index])
    rc = getattr(L, fn_name)(C.byref(args), nb, ix, C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError(f"{fn_name} failed ({rc}): {L.idmvton_last_error().decode()}")


def call_ragged(fn_name, args, seg_nb, seg_index, seg_nk, stream):
    """Invoke an `int f(const args*, const int32_t seg_nb[2], const int32_t* const seg_index[2], const int32_t* const seg_nk[2], void* stream)`
    entry point (the ragged-segment attention launches).  seg_index / seg_nk: two device addresses each, 0 / None = no table for that segment;
    seg_index=None stands for no index table at all."""
    L = lib()
    nb = (i32 * 2)(*seg_nb)
    ix = (vp * 2)(*[int(x) if x else None for x in (seg_index or (0, 0))])
    nk = (vp * 2)(*[int(x) if x else None for x in seg_nk])
    rc = getattr(L, fn_name)(C.byref(args), nb, ix, nk, C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError(f"{fn_name} failed ({rc}): {L.idmvton_last_error().decode()}")


def call_kv_unpack(args, host_desc, stream):
    """Invoke idmvton_kv_unpack(const args*, const desc* host_desc, void* stream); host_desc: a ctypes array of KvUnpackDesc or the address of
    one (what the library validates -- args.desc is its device copy)."""
    L = lib()
    rc = L.idmvton_kv_unpack(C.byref(args), host_desc if isinstance(host_desc, int) else C.cast(host_desc, vp), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError(f"idmvton_kv_unpack failed ({rc}): {L.idmvton_last_error().decode()}")


def _call_kv_table(fn_name, args, host_desc, host_first, stream):
    """Invoke `int f(const args*, const desc* host_desc, const int32_t* host_first, void* stream)`: idmvton_kv_stream, idmvton_kv_fill (a
    descriptor whose src is NULL is a zero run) or idmvton_kv_place (the same, and args.workgroups must be 0: the grid is the table's chunk
    count).  host_desc / host_first: ctypes arrays or the addresses of such (what the library validates -- args.desc / args.first are their
    device copies)."""
    L = lib()
    p = lambda x: x if isinstance(x, int) else C.cast(x, vp)
    rc = getattr(L, fn_name)(C.byref(args), p(host_desc), p(host_first), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError(f"{fn_name} failed ({rc}): {L.idmvton_last_error().decode()}")


call_kv_stream = functools.partial(_call_kv_table, "idmvton_kv_stream")
call_kv_fill = functools.partial(_call_kv_table, "idmvton_kv_fill")
call_kv_place = functools.partial(_call_kv_table, "idmvton_kv_place")


def host_device_ptr(host):
    """idmvton_host_device_ptr: the address under which the device reads the page-locked, mapped host address `host`; RuntimeError with the
    library's message for any other address."""
    L = lib()
    dev = vp()
    rc = L.idmvton_host_device_ptr(C.c_void_p(host), C.byref(dev))
    if rc != 0:
        raise RuntimeError(f"idmvton_host_device_ptr failed ({rc}): {L.idmvton_last_error().decode()}")
    return int(dev.value)
