// kv_unpack.hip -- idmvton_kv_unpack: e4m3 bytes of a packed garment cache -> the 16-bit K / V^T of a persistent set, n independent strided
// 2-D runs in ONE launch driven by a descriptor table (include/idmvton_hip.h).  dst[r][c] = T(e4m3(src[r][c]) * 2^-*exp): an e4m3 value has
// 4 significant bits and |*exp| <= 15, so the product is exact in fp32 and in fp16 / bf16 -- the conversion rounds nothing.
// Bandwidth-bound (1 byte in, 2 out per element): one thread per 16 source bytes, one 16-byte load and two 16-byte stores, KVU_ITEMS of
// them per thread so that a workgroup moves 16 KiB in / 32 KiB out.  Grid (max_chunks, n): block (x, y) owns chunk x of descriptor y and
// leaves at once when that descriptor has fewer chunks.  The descriptor and *exp are workgroup-uniform reads; plain vector stores only.
#include "common.cuh"

#define KVU_THREADS 256
#define KVU_ITEMS 4
#define KVU_CHUNK (KVU_THREADS * KVU_ITEMS)              // 16-byte items of one workgroup

typedef __attribute__((ext_vector_type(2))) float f32x2;
#define GLOBAL_AS __attribute__((address_space(1)))     // pointers read out of the table are generic to the compiler: say that they are global memory

// v_cvt_pk_f32_fp8 gives +0 for the byte 0x80 (measured on the MI355X); the format says -0, and the 16-bit sets must hold the bits the torch
// definition gives.  The byte's sign, moved to bit 31, is OR-ed into the converted value: a no-op for every byte but 0x80.
__device__ __forceinline__ float signed_as(float v, uint32_t sign_at_31) {
    return __uint_as_float(__float_as_uint(v) | (sign_at_31 & 0x80000000u));
}

template <typename T>
__global__ __launch_bounds__(KVU_THREADS) void kv_unpack_kernel(const idmvton_kv_unpack_desc* __restrict__ desc) {
    typedef typename VT<T>::v8 v8;
    const idmvton_kv_unpack_desc d = desc[blockIdx.y];
    const unsigned cpr = (unsigned)d.cols >> 4;                        // 16-byte items per row
    const unsigned total = (unsigned)d.rows * cpr;                     // (the host refuses a run of 2^31 items or more)
    const unsigned base = blockIdx.x * KVU_CHUNK;
    if (base >= total) return;
    int e = *(const GLOBAL_AS int*)d.exp;
    e = e < -7 ? -7 : (e > 15 ? 15 : e);                               // the format's range: 2^-e is a normal fp32 number
    const float s = __int_as_float((127 - e) << 23);
    const GLOBAL_AS uint8_t* src = (const GLOBAL_AS uint8_t*)d.src;
    GLOBAL_AS T* dst = (GLOBAL_AS T*)d.dst;
#pragma unroll
    for (int it = 0; it < KVU_ITEMS; ++it) {
        const unsigned idx = base + it * KVU_THREADS + threadIdx.x;
        if (idx >= total) break;
        const unsigned r = idx / cpr, c = idx - r * cpr;
        const u32x4 ws = *(const GLOBAL_AS u32x4*)(src + (size_t)r * d.lds + c * 16);
        v8 o[2];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t w = ws[q];
            const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
            o[q >> 1][(q & 1) * 4 + 0] = (T)(signed_as(lo[0], w << 24) * s);
            o[q >> 1][(q & 1) * 4 + 1] = (T)(signed_as(lo[1], w << 16) * s);
            o[q >> 1][(q & 1) * 4 + 2] = (T)(signed_as(hi[0], w << 8) * s);
            o[q >> 1][(q & 1) * 4 + 3] = (T)(signed_as(hi[1], w) * s);
        }
        GLOBAL_AS T* p = dst + (size_t)r * d.ldd + c * 16;
        *(GLOBAL_AS v8*)p = o[0];
        *(GLOBAL_AS v8*)(p + 8) = o[1];
    }
}

extern "C" int idmvton_kv_unpack(const idmvton_kv_unpack_args* a, const idmvton_kv_unpack_desc* host_desc, void* stream) {
    CHECK_ARG(a && host_desc && a->desc, IDMVTON_E_ARG, "kv_unpack: null args / descriptor table");
    CHECK_ARG(a->dtype == IDMVTON_F16 || a->dtype == IDMVTON_BF16, IDMVTON_E_DTYPE, "kv_unpack: dtype %d (F16 or BF16)", a->dtype);
    CHECK_ARG(a->n >= 1 && a->n <= 65535, IDMVTON_E_ARG, "kv_unpack: n=%d outside [1, 65535] descriptors", a->n);
    CHECK_ARG(((uintptr_t)a->desc & 15) == 0, IDMVTON_E_ALIGN, "kv_unpack: the device descriptor table is not 16-byte aligned");
    long most = 0;
    for (int i = 0; i < a->n; ++i) {
        const idmvton_kv_unpack_desc* d = host_desc + i;
        CHECK_ARG(d->src && d->dst && d->exp, IDMVTON_E_ARG, "kv_unpack: descriptor %d has a null pointer", i);
        CHECK_ARG(((uintptr_t)d->src & 15) == 0 && ((uintptr_t)d->dst & 15) == 0 && ((uintptr_t)d->exp & 3) == 0, IDMVTON_E_ALIGN,
                  "kv_unpack: descriptor %d: src / dst not 16-byte aligned (or exp not 4-byte aligned)", i);
        CHECK_ARG(d->rows >= 1 && d->cols >= 16 && d->cols % 16 == 0, IDMVTON_E_SHAPE, "kv_unpack: descriptor %d: rows=%d cols=%d (rows >= 1, cols a multiple of 16)",
                  i, d->rows, d->cols);
        CHECK_ARG(d->lds >= d->cols && d->lds % 16 == 0, IDMVTON_E_SHAPE, "kv_unpack: descriptor %d: lds=%d (>= cols=%d, a multiple of 16)", i, d->lds, d->cols);
        CHECK_ARG(d->ldd >= d->cols && d->ldd % 8 == 0, IDMVTON_E_SHAPE, "kv_unpack: descriptor %d: ldd=%d (>= cols=%d, a multiple of 8)", i, d->ldd, d->cols);
        const long items = (long)d->rows * (d->cols >> 4);
        CHECK_ARG(items < (1L << 31), IDMVTON_E_SHAPE, "kv_unpack: descriptor %d: rows=%d x cols=%d is 2^31 16-byte items or more", i, d->rows, d->cols);
        most = items > most ? items : most;
    }
    const long chunks = (most + KVU_CHUNK - 1) / KVU_CHUNK;
    CHECK_ARG(a->max_chunks == chunks, IDMVTON_E_ARG, "kv_unpack: max_chunks=%d, the largest run has %ld chunks of %d 16-byte items", a->max_chunks, chunks, KVU_CHUNK);
    const dim3 grid((unsigned)chunks, (unsigned)a->n), block(KVU_THREADS);
    if (a->dtype == IDMVTON_BF16) hipLaunchKernelGGL((kv_unpack_kernel<bf16_t>), grid, block, 0, (hipStream_t)stream, a->desc);
    else hipLaunchKernelGGL((kv_unpack_kernel<f16_t>), grid, block, 0, (hipStream_t)stream, a->desc);
    CHECK_LAUNCH("kv_unpack");
    return IDMVTON_OK;
}
