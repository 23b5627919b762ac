// guidance.hip -- the per-person CFG step: guidance scale and guidance_rescale per batch element, and the form for the conditional branch
// alone (include/idmvton_hip.h, idmvton_guided_step); the same step with a strength per person (idmvton_person_step): a person that has not
// started yet is skipped; the step of a row plan (idmvton_row_step): a person's eps rows are looked up in a table; and the TryonNet inputs
// of the last two forms (idmvton_pack_input_cond, idmvton_pack_rows).
//
// The arithmetic stands ONCE, in two device bodies that the kernels of the three entries inline.  stats_body: per (chunk of GS_CHUNK pixels,
// person) the four fp64 sums {sum t, sum t^2, sum e, sum e^2} over the chunk's 4 channels -- every thread adds its pixels in index order, a
// wave folds by butterfly (a fixed tree), the four waves are added in wave order -- written to work[(b * nchunks + chunk) * 4 ..] as doubles.
// apply_body: one thread per (person, pixel); thread 0 of a workgroup folds the person's chunks in chunk order and forms the factor.  A
// __global__ kernel decides whether its workgroup returns early and which two eps rows are its person's, nothing else: that an active person
// gets the same bits from every entry is a property of the source, not of copies that agree.  Nothing of this depends on B or on where a
// person stands in the batch, and no value is ever combined by an atomic: the bits of a person's result are a function of its own rows and
// hw.  A product of two fp32 values is exact in fp64, so the only roundings of the statistics are the fp64 additions.
#include "common.cuh"
#include <limits.h>
#include <type_traits>

#define GS_CHUNK 1024                                            // pixels per statistics workgroup: 256 threads x 4 pixels

__device__ __forceinline__ bool rescaled(float phi) { return phi > 0.f; }   // (false for NaN: such a person takes the plain path)

// The arithmetic of cfg_step_kernel (elementwise.hip), spelled out operation by operation: as compiled, that kernel forms the guided eps with
// one FMA, rounds BOTH products of c_x*x + c_eps*eps before adding them (a packed multiply, not an FMA) and adds the noise term with an
// FMA.  Which of these the compiler fuses is its choice there; here nothing is left to it (contraction off, the FMAs explicit), because a
// person without rescale must get that kernel's bits (tests/test_guidance_gpu.py compares them).
__device__ __forceinline__ float cfg_combine(float u, float t, float g) {
#pragma clang fp contract(off)
    return __builtin_fmaf(g, t - u, u);
}
__device__ __forceinline__ float sched_update(float c_x, float c_eps, float sigma, float x, float eps, const float* noise) {
#pragma clang fp contract(off)
    const float p0 = c_x * x, p1 = c_eps * eps;
    float r = p0 + p1;
    if (noise) r = __builtin_fmaf(sigma, *noise, r);
    return r;
}

// Person b's statistics workgroup, its eps rows being ur (unconditional) and cr (conditional).  `a` is any of the three argument structs:
// eps_nhwc, coef, work, B, hw and ldc are read.  A person without rescale has no reduction (uniform over the workgroup).
template <typename T, typename A>
__device__ __forceinline__ void stats_body(const A& a, int b, int ur, int cr) {
    const int tid = threadIdx.x;
    const float g = a.coef[3 + b], phi = a.coef[3 + a.B + b];
    if (!rescaled(phi)) return;
    const T* eu = (const T*)a.eps_nhwc + (size_t)ur * a.hw * a.ldc;
    const T* ec = (const T*)a.eps_nhwc + (size_t)cr * a.hw * a.ldc;
    double st = 0.0, stt = 0.0, se = 0.0, see = 0.0;
#pragma unroll
    for (int i = 0; i < GS_CHUNK / 256; ++i) {
        const int pix = blockIdx.x * GS_CHUNK + i * 256 + tid;
        if (pix < a.hw) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float u = (float)eu[(size_t)pix * a.ldc + c], t = (float)ec[(size_t)pix * a.ldc + c];
                const float e = cfg_combine(u, t, g);
                st += (double)t; stt += (double)t * (double)t;
                se += (double)e; see += (double)e * (double)e;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        st += __shfl_xor(st, o); stt += __shfl_xor(stt, o); se += __shfl_xor(se, o); see += __shfl_xor(see, o);
    }
    __shared__ double red[4][4];
    if ((tid & 63) == 0) { red[tid >> 6][0] = st; red[tid >> 6][1] = stt; red[tid >> 6][2] = se; red[tid >> 6][3] = see; }
    __syncthreads();
    if (tid < 4) {
        double* dst = (double*)a.work + ((size_t)b * gridDim.x + blockIdx.x) * 4;
        dst[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    }
}

// Person b's apply workgroup: one thread per (b, pixel).  both: e = u + g (t - u) from rows ur and cr, rescaled where phi > 0; otherwise
// e = t, row cr alone (ur is not used).  `both` is uniform over the workgroup; a compile-time constant folds as a template argument would.
template <typename T, typename A>
__device__ __forceinline__ void apply_body(const A& a, int nchunks, int b, int ur, int cr, bool both) {
    const int tid = threadIdx.x;
    const int pix = blockIdx.x * 256 + tid;                      // a workgroup lies inside one person
    const float c_x = a.coef[0], c_eps = a.coef[1], sigma = a.coef[2];
    const float g = a.coef[3 + b], phi = a.coef[3 + a.B + b];
    const bool rs = both && rescaled(phi);                       // uniform over the workgroup
    float f = 1.f;
    if (rs) {
        __shared__ float s_f;
        if (tid == 0) {
            const double* part = (const double*)a.work + (size_t)b * nchunks * 4;
            double st = 0.0, stt = 0.0, se = 0.0, see = 0.0;
            for (int k = 0; k < nchunks; ++k) { st += part[4 * k]; stt += part[4 * k + 1]; se += part[4 * k + 2]; see += part[4 * k + 3]; }
            const double n = 4.0 * (double)a.hw;
            const double var_t = (stt - st * st / n) / (n - 1.0), var_e = (see - se * se / n) / (n - 1.0);   // unbiased: torch.std
            s_f = (float)((double)phi * (sqrt(var_t) / sqrt(var_e)) + (1.0 - (double)phi));                  // std(e) == 0: not guarded
        }
        __syncthreads();
        f = s_f;
    }
    if (pix >= a.hw) return;
    const T* ec = (const T*)a.eps_nhwc + ((size_t)cr * a.hw + pix) * a.ldc;
    const T* eu = both ? (const T*)a.eps_nhwc + ((size_t)ur * a.hw + pix) * a.ldc : ec;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const size_t o = ((size_t)b * 4 + c) * a.hw + pix;
        float eps;
        if (both) {
            eps = cfg_combine((float)eu[c], (float)ec[c], g);
            if (rs) eps = eps * f;
        } else {
            eps = (float)ec[c];                                  // the conditional row alone
        }
        a.latents[o] = sched_update(c_x, c_eps, sigma, a.latents[o], eps, a.noise ? a.noise + o : nullptr);
    }
}

// ---- idmvton_guided_step: every person takes the step; rows [uncond B | cond B], or (BR == 1) rows [0, B) the conditional branch alone ----
template <typename T>
__global__ __launch_bounds__(256) void guided_stats_kernel(const idmvton_guided_step_args a) {
    const int b = blockIdx.y;
    stats_body<T>(a, b, b, a.B + b);
}

template <typename T, int BR>
__global__ __launch_bounds__(256) void guided_apply_kernel(const idmvton_guided_step_args a, int nchunks) {
    const int b = blockIdx.y;
    apply_body<T>(a, nchunks, b, b, BR == 2 ? a.B + b : b, BR == 2);
}

// ---- idmvton_person_step: the guided step for the persons that are ACTIVE in this loop step, nothing at all for the DORMANT ones.  The
// coefficient row carries a third per-person column, active[0..B).  A workgroup lies inside one person, so dormancy is uniform over it: both
// kernels return before the first load of that person's eps, latents or noise, before any store and before any barrier -- a skip, not a
// product with zero, so a dormant person's eps rows may hold Inf or NaN and its latents and `work` region keep their bits. ----
__device__ __forceinline__ bool dormant(const float* coef, int B, int b) { return !(coef[3 + 2 * B + b] > 0.f); }   // (NaN: dormant)

template <typename T>
__global__ __launch_bounds__(256) void person_stats_kernel(const idmvton_person_step_args a) {
    const int b = blockIdx.y;
    if (dormant(a.coef, a.B, b)) return;
    stats_body<T>(a, b, b, a.B + b);
}

template <typename T, int BR>
__global__ __launch_bounds__(256) void person_apply_kernel(const idmvton_person_step_args a, int nchunks) {
    const int b = blockIdx.y;
    if (dormant(a.coef, a.B, b)) return;
    apply_body<T>(a, nchunks, b, b, BR == 2 ? a.B + b : b, BR == 2);
}

// ---- idmvton_row_step: a person's eps rows are looked up in a device table {urow[B], crow[B]} instead of implied by [uncond B | cond B].
// crow < 0: dormant -- person_step's skip.  urow < 0 <= crow: e = t, the bodies' arm for the conditional row alone, and no statistics (no
// rescale without guidance).  The three cases are uniform over a workgroup: a person's bits depend neither on R, on B nor on where its
// rows stand. ----
__device__ __forceinline__ int plan_row(const int32_t* rows, int i, int R) {            // clamped to [-1, R - 1]
    const int r = rows[i];
    return r < 0 ? -1 : (r < R ? r : R - 1);
}

template <typename T>
__global__ __launch_bounds__(256) void row_stats_kernel(const idmvton_row_step_args a) {
    const int b = blockIdx.y;
    const int ur = plan_row(a.rows, b, a.R), cr = plan_row(a.rows, a.B + b, a.R);
    if (cr < 0 || ur < 0) return;
    stats_body<T>(a, b, ur, cr);
}

template <typename T>
__global__ __launch_bounds__(256) void row_apply_kernel(const idmvton_row_step_args a, int nchunks) {
    const int b = blockIdx.y;
    const int ur = plan_row(a.rows, b, a.R), cr = plan_row(a.rows, a.B + b, a.R);
    if (cr < 0) return;
    apply_body<T>(a, nchunks, b, ur, cr, ur >= 0);
}

extern "C" int idmvton_guided_step_work_floats(int B, int hw) {
    if (B <= 0 || hw <= 0) return -1;
    const long long n = 8ll * B * ((hw + GS_CHUNK - 1) / GS_CHUNK);
    return n > INT_MAX ? -1 : (int)n;
}

// What the three entries refuse, in one order, under the entry's name.  An entry with a row table has R where the others have `branches`,
// and always runs the statistics.  -> *stats: the call launches the statistics kernel, so `work` was checked.
template <typename A>
static int step_refusals(const char* name, const A* a, bool* stats) {
    constexpr bool table = std::is_same<A, idmvton_row_step_args>::value;
    bool ptrs = a && a->eps_nhwc && a->latents && a->coef;
    if constexpr (table) ptrs = ptrs && a->rows;
    CHECK_ARG(ptrs, IDMVTON_E_ARG, "%s: null pointer", name);
    CHECK_ARG(a->dtype == IDMVTON_F16 || a->dtype == IDMVTON_BF16, IDMVTON_E_DTYPE, "%s: dtype %d", name, a->dtype);
    const bool shape = a->B > 0 && a->B <= 65535 && a->hw > 0 && a->ldc >= 4;
    if constexpr (table) {
        CHECK_ARG(shape && a->R > 0 && a->R <= 65535, IDMVTON_E_SHAPE, "%s: B=%d R=%d hw=%d ldc=%d", name, a->B, a->R, a->hw, a->ldc);
        *stats = true;
    } else {
        CHECK_ARG(a->branches == 1 || a->branches == 2, IDMVTON_E_ARG, "%s: branches=%d (1: the conditional rows alone, 2: [uncond | cond])", name, a->branches);
        CHECK_ARG(shape, IDMVTON_E_SHAPE, "%s: B=%d hw=%d ldc=%d", name, a->B, a->hw, a->ldc);
        *stats = a->branches == 2;
    }
    if (!*stats) return IDMVTON_OK;
    CHECK_ARG(a->work, IDMVTON_E_ARG, "%s: null pointer (work)", name);
    CHECK_ARG(((uintptr_t)a->work & 7) == 0, IDMVTON_E_ALIGN, "%s: work is not 8-byte aligned", name);
    const int need = idmvton_guided_step_work_floats(a->B, a->hw);
    CHECK_ARG(need > 0 && a->work_floats >= need, IDMVTON_E_SHAPE, "%s: work holds %d floats, needs %d", name, a->work_floats, need);
    return IDMVTON_OK;
}

// The launches of a step: the statistics kernel (null: none) over (chunk, person), then the apply kernel over (256 pixels, person).
#define BY_DTYPE(dtype, kernel, ...) ((dtype) == IDMVTON_BF16 ? kernel<bf16_t, ##__VA_ARGS__> : kernel<f16_t, ##__VA_ARGS__>)
template <typename A>
static int step_launch(const char* name, const A& a, void* stream, void (*stats)(const A), void (*apply)(const A, int)) {
    const int nchunks = (a.hw + GS_CHUNK - 1) / GS_CHUNK;
    hipStream_t st = (hipStream_t)stream;
    if (stats) {
        hipLaunchKernelGGL(stats, dim3(nchunks, a.B), dim3(256), 0, st, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return idmvton_set_error(IDMVTON_E_LAUNCH, "%s (statistics): %s", name, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(apply, dim3((a.hw + 255) / 256, a.B), dim3(256), 0, st, a, nchunks);
    CHECK_LAUNCH(name);
    return IDMVTON_OK;
}

extern "C" int idmvton_guided_step(const idmvton_guided_step_args* a, void* stream) {
    bool stats;
    if (const int e = step_refusals("guided_step", a, &stats)) return e;
    return step_launch("guided_step", *a, stream, stats ? BY_DTYPE(a->dtype, guided_stats_kernel) : nullptr,
                       stats ? BY_DTYPE(a->dtype, guided_apply_kernel, 2) : BY_DTYPE(a->dtype, guided_apply_kernel, 1));
}

extern "C" int idmvton_person_step(const idmvton_person_step_args* a, void* stream) {
    bool stats;
    if (const int e = step_refusals("person_step", a, &stats)) return e;
    return step_launch("person_step", *a, stream, stats ? BY_DTYPE(a->dtype, person_stats_kernel) : nullptr,
                       stats ? BY_DTYPE(a->dtype, person_apply_kernel, 2) : BY_DTYPE(a->dtype, person_apply_kernel, 1));
}

extern "C" int idmvton_row_step(const idmvton_row_step_args* a, void* stream) {
    bool stats;
    if (const int e = step_refusals("row_step", a, &stats)) return e;
    return step_launch("row_step", *a, stream, BY_DTYPE(a->dtype, row_stats_kernel), BY_DTYPE(a->dtype, row_apply_kernel));
}

// ---- TryonNet input of a row plan (idmvton_pack_rows): row r = cat(latents[p] | cond[p]), p = row_person[r] read from a device table;
// cond holds one row per PERSON.  pack_input_kernel's body (pack_pixel, common.cuh): a row's bits are those of that person's row there. ----
template <typename T>
__global__ void pack_rows_kernel(const idmvton_pack_rows_args a) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;      // one thread per (row, pixel)
    if (idx >= a.R * a.hw) return;
    const int r = idx / a.hw, pix = idx - r * a.hw;
    int p = a.row_person[r];
    p = p < 0 ? 0 : (p < a.B ? p : a.B - 1);                     // clamped to [0, B - 1]
    pack_pixel<T>(a, idx, p, pix, (size_t)p * a.hw + pix);
}
extern "C" int idmvton_pack_rows(const idmvton_pack_rows_args* a, void* stream) {
    CHECK_ARG(a && a->latents && a->cond && a->out && a->row_person, IDMVTON_E_ARG, "pack_rows: null pointer");
    CHECK_ARG(a->dtype == IDMVTON_F16 || a->dtype == IDMVTON_BF16, IDMVTON_E_DTYPE, "pack_rows: dtype %d", a->dtype);
    CHECK_ARG(a->B > 0 && a->R > 0 && a->hw > 0 && a->cpad >= 13 && (long long)a->R * a->hw <= INT_MAX, IDMVTON_E_SHAPE,
              "pack_rows: B=%d R=%d hw=%d cpad=%d", a->B, a->R, a->hw, a->cpad);
    const int total = a->R * a->hw;
    const dim3 grid((total + 255) / 256), block(256);
    if (a->dtype == IDMVTON_BF16) hipLaunchKernelGGL((pack_rows_kernel<bf16_t>), grid, block, 0, (hipStream_t)stream, *a);
    else hipLaunchKernelGGL((pack_rows_kernel<f16_t>), grid, block, 0, (hipStream_t)stream, *a);
    CHECK_LAUNCH("pack_rows");
    return IDMVTON_OK;
}

// ---- TryonNet input of the conditional branch alone: cat(latents | mask | masked | pose) -> NHWC[cpad], B rows ----
template <typename T>
__global__ void pack_input_cond_kernel(const idmvton_pack_input_args a) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;      // one thread per (b, pixel)
    if (idx >= a.B * a.hw) return;
    const int b = idx / a.hw, pix = idx - b * a.hw;
    pack_pixel<T>(a, idx, b, pix, idx);
}
extern "C" int idmvton_pack_input_cond(const idmvton_pack_input_args* a, void* stream) {
    CHECK_ARG(a && a->latents && a->cond && a->out, IDMVTON_E_ARG, "pack_input_cond: null pointer");
    CHECK_ARG(a->dtype == IDMVTON_F16 || a->dtype == IDMVTON_BF16, IDMVTON_E_DTYPE, "pack_input_cond: dtype %d", a->dtype);
    CHECK_ARG(a->B > 0 && a->hw > 0 && a->cpad >= 13 && (long long)a->B * a->hw <= INT_MAX, IDMVTON_E_SHAPE,
              "pack_input_cond: B=%d hw=%d cpad=%d", a->B, a->hw, a->cpad);
    const int total = a->B * a->hw;
    const dim3 grid((total + 255) / 256), block(256);
    if (a->dtype == IDMVTON_BF16) hipLaunchKernelGGL((pack_input_cond_kernel<bf16_t>), grid, block, 0, (hipStream_t)stream, *a);
    else hipLaunchKernelGGL((pack_input_cond_kernel<f16_t>), grid, block, 0, (hipStream_t)stream, *a);
    CHECK_LAUNCH("pack_input_cond");
    return IDMVTON_OK;
}
