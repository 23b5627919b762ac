// guidance.hip -- the per-person CFG step: guidance scale and guidance_rescale per batch element, and the form for the conditional branch
// alone (include/idmvton_hip.h, idmvton_guided_step); the TryonNet input of that form (idmvton_pack_input_cond); and the same step with a
// strength per person (idmvton_person_step, further down): a person that has not started yet is skipped; and the two edge kernels of a row
// plan (idmvton_row_step, idmvton_pack_rows, further down still): a loop step that runs only the TryonNet rows its persons need.
//
// Two kernels.  guided_stats_kernel: per (chunk of GS_CHUNK pixels, person) the four fp64 sums {sum t, sum t^2, sum e, sum e^2} over the
// chunk's 4 channels -- every thread adds its pixels in index order, a wave folds by butterfly (a fixed tree), the four waves are added in
// wave order -- written to work[(b * nchunks + chunk) * 4 ..] as doubles.  guided_apply_kernel: one thread per (person, pixel); thread 0 of a
// workgroup folds the person's chunks in chunk order and forms the factor.  Nothing of this depends on B or on where a person stands in the
// batch, and no value is ever combined by an atomic: the bits of a person's result are a function of its own rows and hw.
// A product of two fp32 values is exact in fp64, so the only roundings of the statistics are the fp64 additions.
#include "common.cuh"
#include <limits.h>

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

template <typename T>
__global__ __launch_bounds__(256) void guided_stats_kernel(const idmvton_guided_step_args a) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const float g = a.coef[3 + b], phi = a.coef[3 + a.B + b];
    if (!rescaled(phi)) return;                                  // uniform over the workgroup: no reduction for this person
    const T* eu = (const T*)a.eps_nhwc + (size_t)b * a.hw * a.ldc;
    const T* ec = (const T*)a.eps_nhwc + (size_t)(a.B + b) * a.hw * a.ldc;
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

template <typename T, int BR>
__global__ __launch_bounds__(256) void guided_apply_kernel(const idmvton_guided_step_args a, int nchunks) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int pix = blockIdx.x * 256 + tid;                      // one thread per (b, pixel); a workgroup lies inside one person
    const float c_x = a.coef[0], c_eps = a.coef[1], sigma = a.coef[2];
    const float g = a.coef[3 + b], phi = a.coef[3 + a.B + b];
    const bool rs = BR == 2 && rescaled(phi);                    // uniform over the workgroup
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
    const T* eu = (const T*)a.eps_nhwc + ((size_t)b * a.hw + pix) * a.ldc;
    const T* ec = (const T*)a.eps_nhwc + ((size_t)(a.B + b) * a.hw + pix) * a.ldc;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const size_t o = ((size_t)b * 4 + c) * a.hw + pix;
        float eps;
        if (BR == 2) {
            eps = cfg_combine((float)eu[c], (float)ec[c], g);
            if (rs) eps = eps * f;
        } else {
            eps = (float)eu[c];                                  // rows [0, B) are the conditional branch
        }
        a.latents[o] = sched_update(c_x, c_eps, sigma, a.latents[o], eps, a.noise ? a.noise + o : nullptr);
    }
}

extern "C" int idmvton_guided_step_work_floats(int B, int hw) {
    if (B <= 0 || hw <= 0) return -1;
    const long long n = 8ll * B * ((hw + GS_CHUNK - 1) / GS_CHUNK);
    return n > INT_MAX ? -1 : (int)n;
}

extern "C" int idmvton_guided_step(const idmvton_guided_step_args* a, void* stream) {
    CHECK_ARG(a && a->eps_nhwc && a->latents && a->coef, IDMVTON_E_ARG, "guided_step: null pointer");
    CHECK_ARG(a->dtype == IDMVTON_F16 || a->dtype == IDMVTON_BF16, IDMVTON_E_DTYPE, "guided_step: dtype %d", a->dtype);
    CHECK_ARG(a->branches == 1 || a->branches == 2, IDMVTON_E_ARG, "guided_step: branches=%d (1: the conditional rows alone, 2: [uncond | cond])", a->branches);
    CHECK_ARG(a->B > 0 && a->B <= 65535 && a->hw > 0 && a->ldc >= 4, IDMVTON_E_SHAPE, "guided_step: B=%d hw=%d ldc=%d", a->B, a->hw, a->ldc);
    const int nchunks = (a->hw + GS_CHUNK - 1) / GS_CHUNK;
    if (a->branches == 2) {
        CHECK_ARG(a->work, IDMVTON_E_ARG, "guided_step: null pointer (work)");
        CHECK_ARG(((uintptr_t)a->work & 7) == 0, IDMVTON_E_ALIGN, "guided_step: work is not 8-byte aligned");
        const int need = idmvton_guided_step_work_floats(a->B, a->hw);
        CHECK_ARG(need > 0 && a->work_floats >= need, IDMVTON_E_SHAPE, "guided_step: work holds %d floats, needs %d", a->work_floats, need);
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(256), grid((a->hw + 255) / 256, a->B);
    if (a->branches == 2) {
        const dim3 sgrid(nchunks, a->B);
        if (a->dtype == IDMVTON_BF16) hipLaunchKernelGGL((guided_stats_kernel<bf16_t>), sgrid, block, 0, st, *a);
        else hipLaunchKernelGGL((guided_stats_kernel<f16_t>), sgrid, block, 0, st, *a);
        CHECK_LAUNCH("guided_step (statistics)");
        if (a->dtype == IDMVTON_BF16) hipLaunchKernelGGL((guided_apply_kernel<bf16_t, 2>), grid, block, 0, st, *a, nchunks);
        else hipLaunchKernelGGL((guided_apply_kernel<f16_t, 2>), grid, block, 0, st, *a, nchunks);
    } else {
        if (a->dtype == IDMVTON_BF16) hipLaunchKernelGGL((guided_apply_kernel<bf16_t, 1>), grid, block, 0, st, *a, nchunks);
        else hipLaunchKernelGGL((guided_apply_kernel<f16_t, 1>), grid, block, 0, st, *a, nchunks);
    }
    CHECK_LAUNCH("guided_step");
    return IDMVTON_OK;
}

// ---- the per-person step with a strength per person (idmvton_person_step): the guided step for the persons that are ACTIVE in this loop
// step, nothing at all for the DORMANT ones.  The coefficient row carries a third per-person column, active[0..B).  A workgroup lies inside
// one person, so dormancy is uniform over it: both kernels return before the first load of that person's eps, latents or noise and before
// any store -- a skip, not a product with zero, so a dormant person's eps rows may hold Inf or NaN and its latents and `work` region keep
// their bits.  For an active person every operation, in its order, is the one of the guided kernels above (cfg_combine, sched_update, the
// chunked fp64 sums, the chunk-order fold): the same bits.
__device__ __forceinline__ bool dormant(const float* coef, int B, int b) { return !(coef[3 + 2 * B + b] > 0.f); }   // (NaN: dormant)

template <typename T>
__global__ __launch_bounds__(256) void person_stats_kernel(const idmvton_person_step_args a) {
    const int b = blockIdx.y, tid = threadIdx.x;
    if (dormant(a.coef, a.B, b)) return;                         // uniform over the workgroup: before any load of this person's rows
    const float g = a.coef[3 + b], phi = a.coef[3 + a.B + b];
    if (!rescaled(phi)) return;
    const T* eu = (const T*)a.eps_nhwc + (size_t)b * a.hw * a.ldc;
    const T* ec = (const T*)a.eps_nhwc + (size_t)(a.B + b) * a.hw * a.ldc;
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

template <typename T, int BR>
__global__ __launch_bounds__(256) void person_apply_kernel(const idmvton_person_step_args a, int nchunks) {
    const int b = blockIdx.y, tid = threadIdx.x;
    if (dormant(a.coef, a.B, b)) return;                         // uniform over the workgroup: no load, no store, no barrier passed
    const int pix = blockIdx.x * 256 + tid;                      // one thread per (b, pixel); a workgroup lies inside one person
    const float c_x = a.coef[0], c_eps = a.coef[1], sigma = a.coef[2];
    const float g = a.coef[3 + b], phi = a.coef[3 + a.B + b];
    const bool rs = BR == 2 && rescaled(phi);                    // uniform over the workgroup
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
    const T* eu = (const T*)a.eps_nhwc + ((size_t)b * a.hw + pix) * a.ldc;
    const T* ec = (const T*)a.eps_nhwc + ((size_t)(a.B + b) * a.hw + pix) * a.ldc;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const size_t o = ((size_t)b * 4 + c) * a.hw + pix;
        float eps;
        if (BR == 2) {
            eps = cfg_combine((float)eu[c], (float)ec[c], g);
            if (rs) eps = eps * f;
        } else {
            eps = (float)eu[c];                                  // rows [0, B) are the conditional branch
        }
        a.latents[o] = sched_update(c_x, c_eps, sigma, a.latents[o], eps, a.noise ? a.noise + o : nullptr);
    }
}

extern "C" int idmvton_person_step(const idmvton_person_step_args* a, void* stream) {
    CHECK_ARG(a && a->eps_nhwc && a->latents && a->coef, IDMVTON_E_ARG, "person_step: null pointer");
    CHECK_ARG(a->dtype == IDMVTON_F16 || a->dtype == IDMVTON_BF16, IDMVTON_E_DTYPE, "person_step: dtype %d", a->dtype);
    CHECK_ARG(a->branches == 1 || a->branches == 2, IDMVTON_E_ARG, "person_step: branches=%d (1: the conditional rows alone, 2: [uncond | cond])", a->branches);
    CHECK_ARG(a->B > 0 && a->B <= 65535 && a->hw > 0 && a->ldc >= 4, IDMVTON_E_SHAPE, "person_step: B=%d hw=%d ldc=%d", a->B, a->hw, a->ldc);
    const int nchunks = (a->hw + GS_CHUNK - 1) / GS_CHUNK;
    if (a->branches == 2) {
        CHECK_ARG(a->work, IDMVTON_E_ARG, "person_step: null pointer (work)");
        CHECK_ARG(((uintptr_t)a->work & 7) == 0, IDMVTON_E_ALIGN, "person_step: work is not 8-byte aligned");
        const int need = idmvton_guided_step_work_floats(a->B, a->hw);
        CHECK_ARG(need > 0 && a->work_floats >= need, IDMVTON_E_SHAPE, "person_step: work holds %d floats, needs %d", a->work_floats, need);
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(256), grid((a->hw + 255) / 256, a->B);
    if (a->branches == 2) {
        const dim3 sgrid(nchunks, a->B);
        if (a->dtype == IDMVTON_BF16) hipLaunchKernelGGL((person_stats_kernel<bf16_t>), sgrid, block, 0, st, *a);
        else hipLaunchKernelGGL((person_stats_kernel<f16_t>), sgrid, block, 0, st, *a);
        CHECK_LAUNCH("person_step (statistics)");
        if (a->dtype == IDMVTON_BF16) hipLaunchKernelGGL((person_apply_kernel<bf16_t, 2>), grid, block, 0, st, *a, nchunks);
        else hipLaunchKernelGGL((person_apply_kernel<f16_t, 2>), grid, block, 0, st, *a, nchunks);
    } else {
        if (a->dtype == IDMVTON_BF16) hipLaunchKernelGGL((person_apply_kernel<bf16_t, 1>), grid, block, 0, st, *a, nchunks);
        else hipLaunchKernelGGL((person_apply_kernel<f16_t, 1>), grid, block, 0, st, *a, nchunks);
    }
    CHECK_LAUNCH("person_step");
    return IDMVTON_OK;
}

// ---- the step of a ROW PLAN (idmvton_row_step): the person step with the eps rows of a person looked up in a device table {urow[B],
// crow[B]} instead of implied by [uncond B | cond B].  crow < 0: dormant -- person_step's skip, before any load or store.  urow < 0 <= crow:
// e = t, the BR == 1 arm of the apply kernels above.  Both rows: their BR == 2 arm on those two rows.  Every operation, in its order, is
// the one above (cfg_combine, sched_update, the chunked fp64 sums, the chunk-order fold), and a workgroup lies inside one person, so the
// three cases are uniform over it: a person's bits depend neither on R, on B nor on where its rows stand.
__device__ __forceinline__ int plan_row(const int32_t* rows, int i, int R) {            // clamped to [-1, R - 1]
    const int r = rows[i];
    return r < 0 ? -1 : (r < R ? r : R - 1);
}

template <typename T>
__global__ __launch_bounds__(256) void row_stats_kernel(const idmvton_row_step_args a) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int ur = plan_row(a.rows, b, a.R), cr = plan_row(a.rows, a.B + b, a.R);
    if (cr < 0 || ur < 0) return;                                // uniform over the workgroup: dormant, or e = t (no rescale without guidance)
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

template <typename T>
__global__ __launch_bounds__(256) void row_apply_kernel(const idmvton_row_step_args a, int nchunks) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int ur = plan_row(a.rows, b, a.R), cr = plan_row(a.rows, a.B + b, a.R);
    if (cr < 0) return;                                          // uniform over the workgroup: no load, no store, no barrier passed
    const int pix = blockIdx.x * 256 + tid;                      // one thread per (b, pixel); a workgroup lies inside one person
    const float c_x = a.coef[0], c_eps = a.coef[1], sigma = a.coef[2];
    const float g = a.coef[3 + b], phi = a.coef[3 + a.B + b];
    const bool both = ur >= 0;                                   // uniform over the workgroup
    const bool rs = both && rescaled(phi);
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

extern "C" int idmvton_row_step(const idmvton_row_step_args* a, void* stream) {
    CHECK_ARG(a && a->eps_nhwc && a->latents && a->coef && a->rows, IDMVTON_E_ARG, "row_step: null pointer");
    CHECK_ARG(a->dtype == IDMVTON_F16 || a->dtype == IDMVTON_BF16, IDMVTON_E_DTYPE, "row_step: dtype %d", a->dtype);
    CHECK_ARG(a->B > 0 && a->B <= 65535 && a->R > 0 && a->R <= 65535 && a->hw > 0 && a->ldc >= 4, IDMVTON_E_SHAPE,
              "row_step: B=%d R=%d hw=%d ldc=%d", a->B, a->R, a->hw, a->ldc);
    const int nchunks = (a->hw + GS_CHUNK - 1) / GS_CHUNK;
    CHECK_ARG(a->work, IDMVTON_E_ARG, "row_step: null pointer (work)");
    CHECK_ARG(((uintptr_t)a->work & 7) == 0, IDMVTON_E_ALIGN, "row_step: work is not 8-byte aligned");
    const int need = idmvton_guided_step_work_floats(a->B, a->hw);
    CHECK_ARG(need > 0 && a->work_floats >= need, IDMVTON_E_SHAPE, "row_step: work holds %d floats, needs %d", a->work_floats, need);
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(256), grid((a->hw + 255) / 256, a->B), sgrid(nchunks, a->B);
    if (a->dtype == IDMVTON_BF16) hipLaunchKernelGGL((row_stats_kernel<bf16_t>), sgrid, block, 0, st, *a);
    else hipLaunchKernelGGL((row_stats_kernel<f16_t>), sgrid, block, 0, st, *a);
    CHECK_LAUNCH("row_step (statistics)");
    if (a->dtype == IDMVTON_BF16) hipLaunchKernelGGL((row_apply_kernel<bf16_t>), grid, block, 0, st, *a, nchunks);
    else hipLaunchKernelGGL((row_apply_kernel<f16_t>), grid, block, 0, st, *a, nchunks);
    CHECK_LAUNCH("row_step");
    return IDMVTON_OK;
}

// ---- TryonNet input of a row plan (idmvton_pack_rows): row r = cat(latents[p] | cond[p]), p = row_person[r] read from a device table;
// cond holds one row per PERSON.  pack_input_kernel's casts (elementwise.hip): a row's bits are those of that person's row there. ----
template <typename T>
__global__ void pack_rows_kernel(const idmvton_pack_rows_args a) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;      // one thread per (row, pixel)
    if (idx >= a.R * a.hw) return;
    const int r = idx / a.hw, pix = idx - r * a.hw;
    int p = a.row_person[r];
    p = p < 0 ? 0 : (p < a.B ? p : a.B - 1);                     // clamped to [0, B - 1]
    T* o = (T*)a.out + (size_t)idx * a.cpad;
    const T* cond = (const T*)a.cond + ((size_t)p * a.hw + pix) * 9;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = (T)a.latents[((size_t)p * 4 + c) * a.hw + pix];
#pragma unroll
    for (int c = 0; c < 9; ++c) o[4 + c] = cond[c];
    for (int c = 13; c < a.cpad; ++c) o[c] = (T)0.f;
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
    T* o = (T*)a.out + (size_t)idx * a.cpad;
    const T* cond = (const T*)a.cond + (size_t)idx * 9;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = (T)a.latents[((size_t)b * 4 + c) * a.hw + pix];
#pragma unroll
    for (int c = 0; c < 9; ++c) o[4 + c] = cond[c];
    for (int c = 13; c < a.cpad; ++c) o[c] = (T)0.f;
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
