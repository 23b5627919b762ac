// kv_stream.hip -- idmvton_kv_stream: a block of a HOST-RESIDENT garment cache -> the 16-bit K / V^T of a persistent set, n independent strided
// 2-D runs in ONE launch driven by a descriptor table (include/idmvton_hip.h).  idmvton_kv_unpack is built for HBM: a grid of (largest run's
// chunks x descriptors), most workgroups leaving at once, 16 bytes in flight per thread.  A source behind the host link wants the opposite:
// the link is saturated by (rate x latency) bytes in flight, and those should come from FEW, LONG-LIVED workgroups, so that a fill on the side
// stream does not occupy the CUs TryonNet's GEMMs want.  Hence a persistent kernel: `workgroups` workgroups (the host's choice) walk chunks
// blockIdx.x, += gridDim.x of ONE flat chunk list over all descriptors; first[n + 1] -- the exclusive prefix sum of chunks per descriptor,
// built on the host -- maps a chunk to its descriptor by a workgroup-uniform binary search.  A chunk is KVS_CHUNK 16-byte source items, as in
// kv_unpack.  A thread issues ALL its 16-byte loads of a chunk (and, widening, the load of the run's exponent, which may live in host memory
// too) before the first conversion or store, and the loads of its NEXT chunk before it stores the current one.  Neither loads nor stores are
// predicated -- an item index beyond the run is clamped to the run's last item, which such a lane reads and writes again, the same bytes to the
// same place -- and the loop has one uniform exit, so the body is straight-line code: no wait stands between a chunk's stores and the next
// chunk's loads, and the wait before a conversion leaves the other set's loads in flight (checked in the assembly: widening, `s_waitcnt
// vmcnt(13)` after the 5 loads of one set, with 8 stores and the 5 loads of the other set behind the ones it waits for).
// Two modes: WIDEN_E4M3 is kv_unpack's arithmetic, bit for bit (dst = T(e4m3(src) * 2^-clamp(*exp, -7, 15)), the sign of byte 0x80 OR-ed
// back in); COPY moves bytes.  Plain vector loads and stores only.
// idmvton_kv_fill is the same kernel body with FILL = true: a descriptor whose src is NULL is a ZERO RUN, written as a source of all-zero bytes
// would be -- +0 (bits 0x0000) when widening, zero bytes when copying -- WITHOUT any load: kvs_read takes a workgroup-uniform branch on the
// descriptor (it sits in scalar registers) and clears the chunk's registers instead of loading them; neither src nor exp of such a run is
// dereferenced, and kvs_write is unchanged (e4m3 byte 0 times any 2^-e is +0).  That is how a compact garment goes into the front of a larger
// set slot with the zero V^T tail behind it, in one launch.  Data chunks keep the shape above: the branch joins before the sched_barrier and
// the loop is the same straight line of reads and writes with its one uniform exit.  What the join costs: one wait serves both arms, so the
// compiler counts the FEWER operations issued behind the set a conversion needs -- the arm without loads.  Checked in the assembly, widening:
// `s_waitcnt vmcnt(8)` for the exponent (the 8 stores of the write before; kv_stream_kernel has vmcnt(13) there), then `s_waitcnt vmcnt(3)`
// before the first conversion, where kv_stream_kernel has vmcnt(8): after a data chunk's 5 loads that leaves the last 3 of the other set's
// loads in flight, not all 5, and the write drains them as it goes (vmcnt(4), (5), (6)).  The rate does not show it (profiles/LOG.md: the
// same data-only table, 16 workgroups, 56.7 GB/s against kv_stream_kernel's 55.4).  The three kv_stream_kernel instantiations take
// FILL = false, where the branch does not exist: their code is what it was.
#include "common.cuh"

#define KVS_THREADS 256
#define KVS_ITEMS 4
#define KVS_CHUNK (KVS_THREADS * KVS_ITEMS)              // 16-byte items of one chunk: 16 KiB in, 32 KiB (widen) / 16 KiB (copy) out

typedef __attribute__((ext_vector_type(2))) float f32x2;
#define GLOBAL_AS __attribute__((address_space(1)))     // pointers read out of the table are generic to the compiler: say that they are global memory

// (see kv_unpack.hip: v_cvt_pk_f32_fp8 gives +0 for the byte 0x80, the format says -0)
__device__ __forceinline__ float kvs_signed_as(float v, uint32_t sign_at_31) {
    return __uint_as_float(__float_as_uint(v) | (sign_at_31 & 0x80000000u));
}

// chunk q of the flat list -> its descriptor: the largest d with first[d] <= q (every run has at least one chunk: first is strictly increasing)
__device__ __forceinline__ int kvs_find(const int32_t* __restrict__ first, int n, int q) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= q) lo = mid; else hi = mid;
    }
    return lo;
}

struct kvs_chunk {                                       // what a thread holds of one chunk between its loads and its stores
    idmvton_kv_stream_desc d;                            // workgroup-uniform
    unsigned base;                                       // first item of the chunk inside its run
    u32x4 w[KVS_ITEMS];
    int e;
};

template <bool WIDEN, bool FILL>
__device__ __forceinline__ void kvs_read(kvs_chunk& c, const idmvton_kv_stream_desc* __restrict__ desc, const int32_t* __restrict__ first, int n, int q) {
    const int di = kvs_find(first, n, q);
    c.d = desc[di];
    c.base = (unsigned)(q - first[di]) * KVS_CHUNK;
    const unsigned cpr = (unsigned)c.d.cols >> 4;                      // 16-byte items per row
    const unsigned last = (unsigned)c.d.rows * cpr - 1;                // (the host refuses a run of 2^31 items or more)
    const GLOBAL_AS uint8_t* src = (const GLOBAL_AS uint8_t*)c.d.src;
    if (FILL && c.d.src == nullptr) {                                  // a zero run (workgroup-uniform: the descriptor is): no load at all, and
#pragma unroll                                                         // neither src nor exp is looked at -- the chunk a source of zero bytes
        for (int it = 0; it < KVS_ITEMS; ++it) c.w[it] = u32x4{0u, 0u, 0u, 0u};   // would give.  Zero times 2^-e is +0 for every e: c.e takes a value
        c.e = c.d.lds;                                                 // that is NOT a constant, or the compiler folds kvs_write's exponent
                                                                       // arithmetic into both arms and waits for the loaded one right behind the loads
    } else {
#pragma unroll
        for (int it = 0; it < KVS_ITEMS; ++it) {
            unsigned idx = c.base + it * KVS_THREADS + threadIdx.x;
            idx = idx < last ? idx : last;                             // never predicated: an item beyond the run re-reads its last one
            const unsigned r = idx / cpr, col = idx - r * cpr;
            c.w[it] = *(const GLOBAL_AS u32x4*)(src + (size_t)r * c.d.lds + (size_t)col * 16);
        }
        c.e = WIDEN ? *(const GLOBAL_AS int*)c.d.exp : 0;
    }
    // nothing moves across this point: left alone, the scheduler starts converting the OTHER set between the address arithmetic above, and the
    // wait for that set's data then stands before these loads are issued
    __builtin_amdgcn_sched_barrier(0);
}

template <typename T, bool WIDEN>
__device__ __forceinline__ void kvs_write(const kvs_chunk& c) {
    typedef typename VT<T>::v8 v8;
    const unsigned cpr = (unsigned)c.d.cols >> 4;
    const unsigned last = (unsigned)c.d.rows * cpr - 1;
    int e = c.e;
    e = e < -7 ? -7 : (e > 15 ? 15 : e);                               // the format's range: 2^-e is a normal fp32 number
    const float s = __int_as_float((127 - e) << 23);
#pragma unroll
    for (int it = 0; it < KVS_ITEMS; ++it) {
        unsigned idx = c.base + it * KVS_THREADS + threadIdx.x;
        idx = idx < last ? idx : last;                                 // never predicated either: a lane beyond the run holds the run's LAST item
        const unsigned r = idx / cpr, col = idx - r * cpr;             // (kvs_read clamped the same way) and writes it again -- the same bytes
        if (WIDEN) {                                                   // to the same place, inside the run's extent
            v8 o[2];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t w = c.w[it][q];
                const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
                o[q >> 1][(q & 1) * 4 + 0] = (T)(kvs_signed_as(lo[0], w << 24) * s);
                o[q >> 1][(q & 1) * 4 + 1] = (T)(kvs_signed_as(lo[1], w << 16) * s);
                o[q >> 1][(q & 1) * 4 + 2] = (T)(kvs_signed_as(hi[0], w << 8) * s);
                o[q >> 1][(q & 1) * 4 + 3] = (T)(kvs_signed_as(hi[1], w) * s);
            }
            GLOBAL_AS T* p = (GLOBAL_AS T*)c.d.dst + (size_t)r * c.d.ldd + (size_t)col * 16;
            *(GLOBAL_AS v8*)p = o[0];
            *(GLOBAL_AS v8*)(p + 8) = o[1];
        } else {
            *(GLOBAL_AS u32x4*)((GLOBAL_AS uint8_t*)c.d.dst + (size_t)r * c.d.ldd + (size_t)col * 16) = c.w[it];
        }
    }
}

template <typename T, bool WIDEN, bool FILL>
__device__ __forceinline__ void kvs_body(const idmvton_kv_stream_desc* __restrict__ desc, const int32_t* __restrict__ first, int n) {
    const int chunks = first[n];
    const int q0 = blockIdx.x, step = (int)gridDim.x;
    if (q0 >= chunks) return;                                          // only when the host asked for more workgroups than there are chunks
    const int cnt = (chunks - 1 - q0) / step + 1;                      // chunks of this workgroup: q0, q0 + step, ...
    // Two register sets, used in turn, and NO divergent branch anywhere: reads and writes are unpredicated, the loop has one uniform exit at
    // its top and the end of the list is handled after it.  The compiler's wait before a conversion then counts exactly the loads of the other
    // set issued after the ones it needs, and there is no wait between a chunk's stores and the next chunk's loads: two chunks of loads per
    // thread are in flight.  No chunk is read twice.
    kvs_chunk a, b;
    kvs_read<WIDEN, FILL>(a, desc, first, n, q0);
    int i = 1;                                                         // chunks read so far; `a` holds chunk i - 1
    for (; i + 1 < cnt; i += 2) {
        kvs_read<WIDEN, FILL>(b, desc, first, n, q0 + i * step);       // the next chunk's loads are in flight while this one is converted and stored
        kvs_write<T, WIDEN>(a);
        kvs_read<WIDEN, FILL>(a, desc, first, n, q0 + (i + 1) * step);
        kvs_write<T, WIDEN>(b);
    }
    if (i < cnt) {
        kvs_read<WIDEN, FILL>(b, desc, first, n, q0 + i * step);
        kvs_write<T, WIDEN>(a);
        kvs_write<T, WIDEN>(b);
    } else {
        kvs_write<T, WIDEN>(a);
    }
}

template <typename T, bool WIDEN>
__global__ __launch_bounds__(KVS_THREADS) void kv_stream_kernel(const idmvton_kv_stream_desc* __restrict__ desc, const int32_t* __restrict__ first, int n) {
    kvs_body<T, WIDEN, false>(desc, first, n);
}

template <typename T, bool WIDEN>                                      // idmvton_kv_fill: the same body, a NULL src is a zero run
__global__ __launch_bounds__(KVS_THREADS) void kv_fill_kernel(const idmvton_kv_stream_desc* __restrict__ desc, const int32_t* __restrict__ first, int n) {
    kvs_body<T, WIDEN, true>(desc, first, n);
}

// idmvton_kv_place: the same runs, zero runs included, when the sources are in HBM (the staging arena of pipeline.py's _staged_fill).  A short
// HBM-bound pass wants what the persistent body above avoids: the whole machine for as short a time as possible.  So the grid is the flat chunk
// list itself -- first[n] workgroups, workgroup q owns chunk q --: one descriptor search, one kvs_read (a zero run: registers cleared), one
// kvs_write; no loop, no second register set, no idle workgroup.  Lane clamp, arithmetic and zero-run rule are kvs_read's and kvs_write's.
template <typename T, bool WIDEN>
__global__ __launch_bounds__(KVS_THREADS) void kv_place_kernel(const idmvton_kv_stream_desc* __restrict__ desc, const int32_t* __restrict__ first, int n) {
    kvs_chunk c;
    kvs_read<WIDEN, true>(c, desc, first, n, (int)blockIdx.x);         // (the host launches exactly first[n] workgroups)
    kvs_write<T, WIDEN>(c);
}

// What the three entry points check, written once.  `name` is the entry's own in the messages; `zero_ok`: a descriptor whose src is NULL is a zero
// run, not a refusal; `persistent`: workgroups is the grid and lies in [1, 1024], else it must be 0 (the grid is the chunk count).  Returns the
// table's chunk count (>= 1: n >= 1 and every run has a chunk), or the error code (< 0).
static long kvs_check(const idmvton_kv_stream_args* a, const idmvton_kv_stream_desc* host_desc, const int32_t* host_first, const char* name, bool zero_ok, bool persistent) {
    CHECK_ARG(a && host_desc && host_first && a->desc && a->first, IDMVTON_E_ARG, "%s: null args / descriptor table / prefix table", name);
    CHECK_ARG(a->dtype == IDMVTON_F16 || a->dtype == IDMVTON_BF16, IDMVTON_E_DTYPE, "%s: dtype %d (F16 or BF16)", name, a->dtype);
    CHECK_ARG(a->mode == IDMVTON_KVS_WIDEN_E4M3 || a->mode == IDMVTON_KVS_COPY, IDMVTON_E_ARG, "%s: mode %d (IDMVTON_KVS_WIDEN_E4M3 or IDMVTON_KVS_COPY)", name, a->mode);
    CHECK_ARG(a->n >= 1 && a->n <= IDMVTON_KVS_MAX_N, IDMVTON_E_ARG, "%s: n=%d outside [1, %d] descriptors", name, a->n, IDMVTON_KVS_MAX_N);
    CHECK_ARG(!persistent || (a->workgroups >= 1 && a->workgroups <= 1024), IDMVTON_E_ARG, "%s: workgroups=%d outside [1, 1024]", name, a->workgroups);
    CHECK_ARG(persistent || a->workgroups == 0, IDMVTON_E_ARG, "%s: workgroups=%d must be 0 (the grid is the table's chunk count, one workgroup per chunk)", name, a->workgroups);
    CHECK_ARG(((uintptr_t)a->desc & 15) == 0, IDMVTON_E_ALIGN, "%s: the device descriptor table is not 16-byte aligned", name);
    CHECK_ARG(((uintptr_t)a->first & 3) == 0, IDMVTON_E_ALIGN, "%s: the device prefix table is not 4-byte aligned", name);
    const bool widen = a->mode == IDMVTON_KVS_WIDEN_E4M3;
    const int dmul = widen ? 8 : 16;                                   // ldd: elements when widening, bytes when copying
    long chunks = 0;
    for (int i = 0; i < a->n; ++i) {
        const idmvton_kv_stream_desc* d = host_desc + i;
        const bool zero = zero_ok && d->src == nullptr;                // a zero run: exp and lds are not looked at
        CHECK_ARG((d->src || zero) && d->dst && (zero || d->exp || !widen), IDMVTON_E_ARG, "%s: descriptor %d has a null pointer%s", name, i,
                  !zero_ok ? "" : zero ? " (dst of a zero run)" : " (dst, or exp of a data run)");
        CHECK_ARG(((uintptr_t)d->src & 15) == 0 && ((uintptr_t)d->dst & 15) == 0 && (zero || !widen || ((uintptr_t)d->exp & 3) == 0), IDMVTON_E_ALIGN,
                  "%s: descriptor %d: src / dst not 16-byte aligned (or exp not 4-byte aligned)", name, i);
        CHECK_ARG(d->rows >= 1 && d->cols >= 16 && d->cols % 16 == 0, IDMVTON_E_SHAPE, "%s: descriptor %d: rows=%d cols=%d (rows >= 1, cols a multiple of 16)",
                  name, i, d->rows, d->cols);
        CHECK_ARG(zero || (d->lds >= d->cols && d->lds % 16 == 0), IDMVTON_E_SHAPE, "%s: descriptor %d: lds=%d (>= cols=%d, a multiple of 16)", name, i, d->lds, d->cols);
        CHECK_ARG(d->ldd >= d->cols && d->ldd % dmul == 0, IDMVTON_E_SHAPE, "%s: descriptor %d: ldd=%d (>= cols=%d, a multiple of %d)", name, i, d->ldd, d->cols, dmul);
        const long items = (long)d->rows * (d->cols >> 4);
        CHECK_ARG(items < (1L << 31), IDMVTON_E_SHAPE, "%s: descriptor %d: rows=%d x cols=%d is 2^31 16-byte items or more", name, i, d->rows, d->cols);
        CHECK_ARG(host_first[i] == chunks, IDMVTON_E_ARG, "%s: host_first[%d]=%d, the runs before descriptor %d have %ld chunks of %d 16-byte items",
                  name, i, host_first[i], i, chunks, KVS_CHUNK);
        chunks += (items + KVS_CHUNK - 1) / KVS_CHUNK;
        CHECK_ARG(chunks < (1L << 31), IDMVTON_E_SHAPE, "%s: 2^31 chunks or more up to descriptor %d", name, i);
    }
    CHECK_ARG(host_first[a->n] == chunks, IDMVTON_E_ARG, "%s: host_first[%d]=%d, the table has %ld chunks of %d 16-byte items", name, a->n, host_first[a->n], chunks, KVS_CHUNK);
    return chunks;
}

// Launches the instantiation a call asks for, out of the three of one kernel template (COPY = <bf16_t, false>: copying never looks at T).
typedef void (*kvs_kernel_t)(const idmvton_kv_stream_desc*, const int32_t*, int);
template <kvs_kernel_t COPY, kvs_kernel_t BF16, kvs_kernel_t F16>
static int kvs_launch(const idmvton_kv_stream_args* a, long grid, void* stream, const char* name) {
    const kvs_kernel_t k = a->mode == IDMVTON_KVS_COPY ? COPY : a->dtype == IDMVTON_BF16 ? BF16 : F16;
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(KVS_THREADS), 0, (hipStream_t)stream, a->desc, a->first, a->n);
    CHECK_LAUNCH(name);
    return IDMVTON_OK;
}
#define KVS_OF(K) K<bf16_t, false>, K<bf16_t, true>, K<f16_t, true>

extern "C" int idmvton_kv_stream(const idmvton_kv_stream_args* a, const idmvton_kv_stream_desc* host_desc, const int32_t* host_first, void* stream) {
    const long chunks = kvs_check(a, host_desc, host_first, "kv_stream", false, true);
    return chunks < 0 ? (int)chunks : kvs_launch<KVS_OF(kv_stream_kernel)>(a, a->workgroups, stream, "kv_stream");
}

extern "C" int idmvton_kv_fill(const idmvton_kv_stream_args* a, const idmvton_kv_stream_desc* host_desc, const int32_t* host_first, void* stream) {
    const long chunks = kvs_check(a, host_desc, host_first, "kv_fill", true, true);
    return chunks < 0 ? (int)chunks : kvs_launch<KVS_OF(kv_fill_kernel)>(a, a->workgroups, stream, "kv_fill");
}

extern "C" int idmvton_kv_place(const idmvton_kv_stream_args* a, const idmvton_kv_stream_desc* host_desc, const int32_t* host_first, void* stream) {
    const long chunks = kvs_check(a, host_desc, host_first, "kv_place", true, false);
    return chunks < 0 ? (int)chunks : kvs_launch<KVS_OF(kv_place_kernel)>(a, chunks, stream, "kv_place");   // one workgroup per chunk
}

extern "C" int idmvton_host_device_ptr(const void* host, void** dev) {
    CHECK_ARG(host && dev, IDMVTON_E_ARG, "host_device_ptr: null argument");
    *dev = nullptr;
    const hipError_t e = hipHostGetDevicePointer(dev, const_cast<void*>(host), 0);
    if (e != hipSuccess || !*dev) {
        (void)hipGetLastError();                                       // the refusal is reported here, not by the next launch check
        *dev = nullptr;
        return idmvton_set_error(IDMVTON_E_ARG, "host_device_ptr: %p is not page-locked, device-mapped host memory (%s): allocate with pin_memory=True",
                                 host, hipGetErrorString(e));
    }
    return IDMVTON_OK;
}
