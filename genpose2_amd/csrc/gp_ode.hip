// Probability-flow ODE sampler on device: Dormand-Prince 5(4) stages fused with the score heads.
//
// Reference: cond_ode_sampler (networks/gf_algorithms/samplers.py:180-258) hands the float64 state
// to scipy solve_ivp(method="RK45") and pays a device->host and host->device copy per right-hand
// side. Here an RK45 stage is a fused kernel body: the stage combination y + (sum_j a_j K_j) * h (fp64,
// scipy rk.py rk_step order) is formed in the prologue, cast to the fp32 pose the score model sees
// (samplers.py:210), the head trunk evaluates the score, and the epilogue writes
// K_s = -(0.5 g(t)^2) * score in fp64 (samplers.py:216). The last stage of an attempted step also
// writes y_new and the per-workgroup sum of (err / scale)^2 of scipy's error estimator
// (_estimate_error_norm, rk.py); ode_norm_kernel reduces it in a fixed order. The step
// controller's scalars stay on the host (genpose2_amd/ode.py): one 8-byte read per attempt. The
// device-controlled attempts (gp_ode_auto_attempt) run all six stages of an attempt in one launch
// (ode_attempt_kernel); the host-controlled ones launch each stage (ode_stage_kernel). What the energy agent's
// stages (gp_ode_energy.hip) and the per-object likelihood (gp_like_object.hip) share with these is in gp_ode.h:
// the entries here hand ode_rhs_once, ode_attempt_host and ode_run_stages their stage launch (ode_launch_stage,
// like_launch_stage) and keep only their own checks.
#include <chrono>
#include <cstddef>
#include <cstdlib>
#include <mutex>
#include <utility>
#include <vector>

#include "gp_ode.h"

// One RK45 stage for the workgroup's rows. MODE 0: stage derivative. MODE 1: last stage of an attempt
// (y_new, K_6, error partials). y_in = y + (sum_{j<nk} acoef_j K_j) h, K_out = coef * score(f32(y_in), t).
template <int MODE, int PL, int NT>
__device__ __forceinline__ void ode_stage_body(const OdeStageArgs& a, const double* y, const double* const* kin,
                                               const double* acoef, int nk, double h, double coef, float sigma,
                                               const float* tproj, double* kout, double* ynew,
                                               HeadSmem<NT, EVAL_WV, PL>& sm, int* obj, double* y0s, double* y1s,
                                               double* esq, const SplitScalars& hs) {
    constexpr int ROWS = 16 * NT;
    constexpr int NTH = EVAL_WV * 64;
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * ROWS;
    stage_small_weights(a.w, sm);
    for (int i = tid; i < ROWS * 16; i += NTH) {
        const int c = i >> 4, j = i & 15;
        const int r = r0 + c;
        float xv = 0.f;
        if (r < a.rows && j < 9) {
            const size_t e = (size_t)r * 9 + j;
            const double yv = y[e];
            const double yi = nk > 0 ? ode_stage_in(kin, acoef, nk, h, e, yv) : yv;
            xv = (float)yi;   // torch.tensor(x, dtype=torch.float32) (samplers.py:210)
            if (MODE == 1) {
                y0s[c * 9 + j] = yv;
                y1s[c * 9 + j] = yi;
                ynew[e] = yi;
            }
        }
        sm.xin[i] = xv;
    }
    if (tid < ROWS) obj[tid] = obj_of_row(r0 + tid, a.rows, a.kper);
    run_head_trunk(a.w, a.pobj, tproj, obj, sm, 0, hs);
    double sq = 0.0;   // this thread's (err/scale)^2 terms, its elements in increasing order
    for (int e9 = tid; e9 < ROWS * 9; e9 += NTH) {
#pragma clang fp contract(off)
        const int c = e9 / 9, o = e9 - c * 9;
        const int r = r0 + c;
        if (r < a.rows) {
            const size_t e = (size_t)r * 9 + o;
            const float s = fdiv(head_out(sm, c, o), fadd(sigma, 1e-7f));
            const double kv = coef * (double)s;
            kout[e] = kv;
            if (MODE == 1) {
                const double er = ode_err_term(a, kin, kv, h, e, y0s[c * 9 + o], y1s[c * 9 + o]);
                sq += er * er;
            }
        }
    }
    if (MODE == 1) ode_block_partial(sq, esq, &a.part[a.part_off + blockIdx.x]);
}

// MODE 0: stage derivative. MODE 1: last stage of an attempt (y_new, K_6, error partials).
// NT column tiles of 16 candidates per workgroup (head_pick_nt: 32 / 64 candidates from 4097 / 8193 rows
// with the split-f16 trunk, as the PC step).
template <int MODE, int PL, int NT>   // PL 0: exact fp32 GEMMs, X3P: f16x3
__global__ __launch_bounds__(EVAL_WV * 64) void ode_stage_kernel(OdeStageArgs a) {
    constexpr int ROWS = 16 * NT;
    constexpr int NTH = EVAL_WV * 64;
    __shared__ HeadSmem<NT, EVAL_WV, PL> sm;
    __shared__ int obj[ROWS];
    __shared__ double y0s[ROWS * 9], y1s[ROWS * 9], esq[NTH];
    const SplitScalars hs = load_split_scalars<PL>(a.w);
    const double* y = a.y;
    const double* kin[ODE_NK];
#pragma unroll
    for (int j = 0; j < ODE_NK; ++j) kin[j] = a.k[j];
    double h = a.h, coef = a.coef;
    float sigma = a.sigma;
    const float* tproj = a.tproj;
    double* kout = a.kout;
    double* ynew = a.ynew;
    if (a.ctl != nullptr) {   // device-controlled: skip when no attempt was prepared
        const OdeCtl* c = a.ctl;
        if (!c->active) return;
        y = a.ybuf[c->yi];
#pragma unroll
        for (int j = 0; j < ODE_NK; ++j) kin[j] = a.kbuf[c->kidx[j]];
        h = c->h;
        coef = c->coef[a.stage - 1];
        sigma = c->sig[a.stage - 1];
        tproj = a.tproj6 + (size_t)(a.stage - 1) * 768;
        kout = a.kbuf[c->kidx[a.stage]];
        ynew = a.ybuf[c->yi ^ 1];
    }
    ode_stage_body<MODE, PL, NT>(a, y, kin, a.a, a.nk, h, coef, sigma, tproj, kout, ynew, sm, obj, y0s, y1s, esq, hs);
}

// A whole device-controlled attempt in one launch: the six stages run back to back in every workgroup
// (a stage needs only its own rows' earlier stages, so no grid-wide step separates them -- only the
// controller's accept / reject between attempts does). Stage s combines K_0..K_{s-1} with tableau row
// A[s] (stage 6: B, y_new and the error partials), exactly as the six stage launches do: bit-identical,
// without five kernel boundaries (each ~3 us of tail, boundary and refill at config 4). The K_s a stage
// writes are read back by other threads of the workgroup after the stage's barrier (the workgroup-scope
// release / acquire of __syncthreads orders the global stores before those loads).
template <int PL, int NT>
__global__ __launch_bounds__(EVAL_WV * 64) void ode_attempt_kernel(OdeStageArgs a, OdeTableau tb) {
    constexpr int ROWS = 16 * NT;
    constexpr int NTH = EVAL_WV * 64;
    __shared__ HeadSmem<NT, EVAL_WV, PL> sm;
    __shared__ int obj[ROWS];
    __shared__ double y0s[ROWS * 9], y1s[ROWS * 9], esq[NTH];
    __shared__ double tab[42];
    __shared__ const double* kin[ODE_NK];
    const OdeCtl* c = a.ctl;
    if (!c->active) return;
    ode_attempt_to_lds(a, c, tb, tab, kin);
    const double* y = a.ybuf[c->yi];
    const double h = c->h;
    __syncthreads();
    for (int s = 1; s < 6; ++s) {
        if (s > 1) __syncthreads();   // stage s-1's K stores and its reads of the staged weights are done
        // per stage (L2-resident): held across the stages they would add to the trunk's register peak
        const SplitScalars hs = load_split_scalars<PL>(a.w);
        ode_stage_body<0, PL, NT>(a, y, kin, tab + s * 6, s, h, c->coef[s - 1], c->sig[s - 1],
                                  a.tproj6 + (size_t)(s - 1) * 768, const_cast<double*>(kin[s]), nullptr, sm, obj,
                                  y0s, y1s, esq, hs);
    }
    __syncthreads();
    const SplitScalars hs = load_split_scalars<PL>(a.w);
    ode_stage_body<1, PL, NT>(a, y, kin, tab + 36, 6, h, c->coef[5], c->sig[5], a.tproj6 + (size_t)5 * 768,
                              const_cast<double*>(kin[6]), a.ybuf[c->yi ^ 1], sm, obj, y0s, y1s, esq, hs);
}

// Stage-kernel launch of `nt` column tiles per workgroup (1 for the exact-fp32 trunk); last: MODE 1. what: the
// launch check's label, or null where the caller checks once behind a later launch (stages 1..5 of an attempt).
static int ode_launch_stage(const OdeStageArgs& a, int nt, bool last, const char* what, hipStream_t st) {
    const int nwg = (a.rows + 16 * nt - 1) / (16 * nt);
    const dim3 grid(nwg), blk(EVAL_WV * 64);
    head_dispatch(a.w.pe2_h ? X3P : 0, nt, [&](auto pl, auto ntc) {
        if (last)
            hipLaunchKernelGGL((ode_stage_kernel<1, pl.value, ntc.value>), grid, blk, 0, st, a);
        else
            hipLaunchKernelGGL((ode_stage_kernel<0, pl.value, ntc.value>), grid, blk, 0, st, a);
    });
    return what ? gp_check_launch(what) : GP_OK;
}

static int ode_nt(const gp_head_weights* w, int rows) { return head_pick_nt(rows, w->pe2_h != nullptr); }
static int ode_nwg(const gp_head_weights* w, int rows) {
    const int nt = ode_nt(w, rows);
    return (rows + 16 * nt - 1) / (16 * nt);
}

// ============================================================================ likelihood stages
// cond_ode_likelihood (samplers.py:25-110): the augmented state y = [x (9R) | logp (R)] (scipy's flat layout),
// d logp_r / dt = coef * eps_r . (d score_r / d x_r) eps_r with the constant direction eps (R,9). A workgroup
// holds NP primal column tiles and their NP tangent tiles (the JVP trunk, gp_head.h): entry o < 9 of row r is
// x_r[o] at y[9 r + o], entry 9 is logp_r at y[9 R + r]. Otherwise ode_stage_body: same stage combination, same
// error terms (over all ten entries of a row), same fixed summation order of the workgroup partial.
template <int MODE, int PL, int NP>
__global__ __launch_bounds__(EVAL_WV * 64) void like_stage_kernel(OdeStageArgs a, const float* __restrict__ eps) {
    constexpr int NT = 2 * NP;
    constexpr int ROWS = 16 * NP;     // rows (candidates) of this workgroup
    constexpr int NTH = EVAL_WV * 64;
    __shared__ HeadSmem<NT, EVAL_WV, PL> sm;
    __shared__ int obj[2 * ROWS];
    __shared__ double y0s[ROWS * 10], y1s[ROWS * 10], esq[EVAL_WV];
    const SplitScalars hs = load_split_scalars<PL>(a.w);
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * ROWS;
    const double h = a.h;
    const size_t n9 = (size_t)a.rows * 9;
    stage_small_weights(a.w, sm);
    auto stage_in = [&](size_t e, double yv) { return a.nk > 0 ? ode_stage_in(a.k, a.a, a.nk, h, e, yv) : yv; };
    for (int i = tid; i < 2 * ROWS * 16; i += NTH) {
        const int c = i >> 4, j = i & 15;
        float xv = 0.f;
        if (c < ROWS) {
            const int r = r0 + c;
            if (r < a.rows && j < 9) {
                const size_t e = (size_t)r * 9 + j;
                const double yv = a.y[e];
                const double yi = stage_in(e, yv);
                xv = (float)yi;   // torch.tensor(x, dtype=torch.float32) (samplers.py:83)
                if (MODE == 1) {
                    y0s[c * 10 + j] = yv;
                    y1s[c * 10 + j] = yi;
                    a.ynew[e] = yi;
                }
            }
        } else {
            const int r = r0 + c - ROWS;
            if (r < a.rows && j < 9) xv = eps[(size_t)r * 9 + j];
        }
        sm.xin[i] = xv;
    }
    if (MODE == 1 && tid < ROWS && r0 + tid < a.rows) {   // logp: not an input of the RHS, only of y_new and the error
        const size_t e = n9 + (size_t)(r0 + tid);
        const double yv = a.y[e];
        const double yi = stage_in(e, yv);
        y0s[tid * 10 + 9] = yv;
        y1s[tid * 10 + 9] = yi;
        a.ynew[e] = yi;
    }
    if (tid < 2 * ROWS) obj[tid] = obj_of_row(r0 + (tid < ROWS ? tid : tid - ROWS), a.rows, a.kper);
    if constexpr (PL != 0)
        head_trunk_x3<NT, EVAL_WV, false, true>(a.w, a.pobj, a.tproj, obj, sm, 0, hs);
    else
        head_trunk<NT, EVAL_WV, true>(a.w, a.pobj, a.tproj, obj, sm);
    double sq = 0.0;   // this thread's (err/scale)^2 terms, its elements in increasing order
    const float den = fadd(a.sigma, 1e-7f);
    for (int e10 = tid; e10 < ROWS * 10; e10 += NTH) {
#pragma clang fp contract(off)
        const int c = e10 / 10, o = e10 - c * 10;
        const int r = r0 + c;
        if (r < a.rows) {
            const size_t e = o < 9 ? (size_t)r * 9 + o : n9 + (size_t)r;
            float s;
            if (o < 9) {
                s = fdiv(head_out(sm, c, o), den);
            } else {   // eps . (J eps): nine fp32 products, each rounded on its own, summed in order
                s = 0.f;
#pragma unroll
                for (int j = 0; j < 9; ++j)
                    s = fadd(s, fmul(ld1(&sm.xin[(ROWS + c) * 16 + j]), fdiv(head_out<true>(sm, ROWS + c, j), den)));
            }
            const double kv = a.coef * (double)s;
            a.kout[e] = kv;
            if (MODE == 1) {
                const double er = ode_err_term(a, a.k, kv, h, e, y0s[e10], y1s[e10]);
                sq += er * er;
            }
        }
    }
    // part_off stays out of it: the likelihood has no global-batch shards (host-side it is always 0 here)
    if (MODE == 1) ode_block_partial(sq, esq, &a.part[blockIdx.x]);
}

// Primal column tiles per workgroup of the likelihood stages: a workgroup streams the GEMM weights once for its
// primal and tangent tiles together, so the split trunk takes two primal tiles (the 64-column workgroup of the
// sampler's widest tiling) once 16-row workgroups no longer fit one pass of the CUs.
static int like_np(const gp_head_weights* w, int rows) {
    return (w->pe2_h != nullptr && rows >= PC_SPLIT_NT2_MIN) ? 2 : 1;
}

static int like_launch_stage(const OdeStageArgs& a, const float* eps, int np, bool last, const char* what,
                             hipStream_t st) {
    const dim3 grid((a.rows + 16 * np - 1) / (16 * np)), blk(EVAL_WV * 64);
    head_dispatch<2>(a.w.pe2_h ? X3P : 0, np, [&](auto pl, auto npc) {
        if (last)
            hipLaunchKernelGGL((like_stage_kernel<1, pl.value, npc.value>), grid, blk, 0, st, a, eps);
        else
            hipLaunchKernelGGL((like_stage_kernel<0, pl.value, npc.value>), grid, blk, 0, st, a, eps);
    });
    return what ? gp_check_launch(what) : GP_OK;
}

// Sum of part[0..n) by a 256-thread workgroup in a fixed order (strided per-thread sums, xor
// shuffles within each wave, the four wave sums in wave order): every caller that reduces the same
// partials gets the same bits. `red` is 4 doubles of LDS.
__device__ __forceinline__ double block_sum_f64(const double* __restrict__ part, int n, double* red) {
    double t = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) t += part[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// out[0] = sqrt(sum(part[0..n))) / sqrt(count): scipy's RMS norm over the error partials.
__global__ __launch_bounds__(256) void ode_norm_kernel(const double* __restrict__ part, int n, double count,
                                                       double* __restrict__ out) {
    __shared__ double red[4];
    const double t = block_sum_f64(part, n, red);
    if (threadIdx.x == 0) out[0] = sqrt(t) / sqrt(count);
}

// select_initial_step norms (scipy _ivp/common.py): scale = atol + |y0| rtol;
// f1 == NULL: out[0] = rms(y0 / scale), out[1] = rms(f0 / scale); else out[2] = rms((f1 - f0) / scale).
__global__ __launch_bounds__(1024) void ode_init_norms_kernel(const double* __restrict__ y0,
                                                              const double* __restrict__ f0,
                                                              const double* __restrict__ f1, long long n,
                                                              double atol, double rtol, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double r0[16], r1[16];
    double s0 = 0.0, s1 = 0.0;
    // each thread's elements i = tid + 1024 j in increasing j, as one load per step would add them; the loads of
    // IL consecutive steps are issued together (a load per dependent add waited a full memory round trip each:
    // 76 -> 42 us per call at R = 12,800; the rest is the fp64 divisions of one workgroup)
    constexpr int IL = 8;
    long long i0 = threadIdx.x;
    for (; i0 + 1024LL * (IL - 1) < n; i0 += 1024LL * IL) {
        double yv[IL], fa[IL], fb[IL];
#pragma unroll
        for (int j = 0; j < IL; ++j) {
            yv[j] = y0[i0 + 1024LL * j];
            fa[j] = f0[i0 + 1024LL * j];
        }
        if (f1 != nullptr) {
#pragma unroll
            for (int j = 0; j < IL; ++j) fb[j] = f1[i0 + 1024LL * j];
        } else {
#pragma unroll
            for (int j = 0; j < IL; ++j) fb[j] = 0.0;
        }
#pragma unroll
        for (int j = 0; j < IL; ++j) {
            const double sc = atol + fabs(yv[j]) * rtol;
            if (f1 == nullptr) {
                const double u = yv[j] / sc, v = fa[j] / sc;
                s0 += u * u;
                s1 += v * v;
            } else {
                const double v = (fb[j] - fa[j]) / sc;
                s0 += v * v;
            }
        }
    }
    for (long long i = i0; i < n; i += 1024) {
        const double sc = atol + fabs(y0[i]) * rtol;
        if (f1 == nullptr) {
            const double u = y0[i] / sc, v = f0[i] / sc;
            s0 += u * u;
            s1 += v * v;
        } else {
            const double v = (f1[i] - f0[i]) / sc;
            s0 += v * v;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s0 += __shfl_xor(s0, off, 64);
        s1 += __shfl_xor(s1, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        r0[threadIdx.x >> 6] = s0;
        r1[threadIdx.x >> 6] = s1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 16; ++i) {
            r0[0] += r0[i];
            r1[0] += r1[i];
        }
    }
    if (threadIdx.x == 0) {
        const double rn = sqrt((double)n);
        if (f1 == nullptr) {
            out[0] = sqrt(r0[0]) / rn;
            out[1] = sqrt(r1[0]) / rn;
        } else {
            out[2] = sqrt(r0[0]) / rn;
        }
    }
}

// Dense output of an accepted step (scipy RkDenseOutput, rk.py): for each requested t_eval point
// te = tev[i], x = (te - t_old) / h, p = cumprod([x, x, x, x]), y = h * (Q p) + y_old with
// Q = K^T P. Writes out[(i - i_base) * n + e] for i in [i0, i1).
struct OdeDenseArgs {
    const double* k[ODE_NK];
    double P[ODE_NK][4];
    const double* y_old;
    const double* tev;
    int i0, i1, i_base;
    double t_old, h;
    double* out;
    long long n;
    int reverse;   // out row = (i_base - i) instead of (i - i_base)
};

__global__ __launch_bounds__(256) void ode_dense_kernel(OdeDenseArgs a) {
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.n) return;
    double Q[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        double acc = a.k[0][e] * a.P[0][m];
        for (int j = 1; j < ODE_NK; ++j) acc = acc + a.k[j][e] * a.P[j][m];
        Q[m] = acc;
    }
    const double yo = a.y_old[e];
    for (int i = a.i0; i < a.i1; ++i) {
        const double x = (a.tev[i] - a.t_old) / a.h;
        const double p1 = x, p2 = p1 * x, p3 = p2 * x, p4 = p3 * x;
        const double d = ((Q[0] * p1 + Q[1] * p2) + Q[2] * p3) + Q[3] * p4;
        const long long row = a.reverse ? (long long)(a.i_base - i) : (long long)(i - a.i_base);
        a.out[row * a.n + e] = a.h * d + yo;
    }
}

// Final denoise (samplers.py:240-249) + epilogue: grad = score(float(x), eps) in fp32,
// mean_x = x + (0 - g^2 grad) * c (fp32 product, fp64 sum), then GS of [:6], + pts_center, quaternion
// (posenet_agent.py:554-556). Writes pose (R,9) fp64 and q (R,7) fp64. The score runs on the stage kernels'
// trunk and tile (f16x3, 64 candidates per workgroup at R >= 8193; exact fp32 without the f16 planes).

template <int PL, int NT>   // PL 0: exact fp32 trunk, X3P: f16x3 (the stage kernels' arithmetic)
__global__ __launch_bounds__(EVAL_WV * 64) void ode_denoise_kernel(OdeDenoiseArgs a) {
    constexpr int ROWS = 16 * NT;
    constexpr int NTH = EVAL_WV * 64;
    __shared__ HeadSmem<NT, EVAL_WV, PL> sm;
    __shared__ int obj[ROWS];
    __shared__ double xm[ROWS * 9];
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * ROWS;
    const SplitScalars hs = load_split_scalars<PL>(a.w);
    stage_small_weights(a.w, sm);
    for (int i = tid; i < ROWS * 16; i += NTH) {
        const int c = i >> 4, j = i & 15;
        const int r = r0 + c;
        sm.xin[i] = (r < a.rows && j < 9) ? (float)a.x[(size_t)r * 9 + j] : 0.f;
    }
    if (tid < ROWS) obj[tid] = obj_of_row(r0 + tid, a.rows, a.kper);
    run_head_trunk(a.w, a.pobj, a.tproj, obj, sm, 0, hs);
    for (int e9 = tid; e9 < ROWS * 9; e9 += NTH) {
#pragma clang fp contract(off)
        const int c = e9 / 9, o = e9 - c * 9;
        const int r = r0 + c;
        if (r < a.rows) {
            const float grad = fdiv(head_out(sm, c, o), fadd(a.sigma, 1e-7f));
            const float drift = 0.0f - a.g2 * grad;
            xm[e9] = a.x[(size_t)r * 9 + o] + (double)(drift * a.step);
        }
    }
    __syncthreads();
    if (tid < ROWS && r0 + tid < a.rows) {
        const int r = r0 + tid;
        double v[9], qq[4];
#pragma unroll
        for (int j = 0; j < 9; ++j) v[j] = xm[tid * 9 + j];
        gram_schmidt6<double>(v);
        const float* cen = a.center + (size_t)obj[tid] * 3;
        v[6] += (double)ld1(cen);
        v[7] += (double)ld1(cen + 1);
        v[8] += (double)ld1(cen + 2);
        quat_from_gs<double>(v, qq);
#pragma unroll
        for (int j = 0; j < 9; ++j) a.pose[(size_t)r * 9 + j] = v[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) a.q[(size_t)r * 7 + j] = qq[j];
#pragma unroll
        for (int j = 0; j < 3; ++j) a.q[(size_t)r * 7 + 4 + j] = v[6 + j];
    }
}

// Time rows of up to 6 stage times passed by value (no host->device copy per attempt); each row is
// split over ODE_ROW_CHUNKS workgroups.
#define ODE_ROW_CHUNKS 8
struct OdeTimes {
    float t[6];
};
__global__ __launch_bounds__(HT) void ode_time_rows_kernel(gp_head_weights w, OdeTimes tv, float* __restrict__ out) {
    __shared__ float emb[128];
    __shared__ float tf[128];
    constexpr int PER = 768 / ODE_ROW_CHUNKS;
    time_row(w, tv.t[blockIdx.x], emb, tf, out + (size_t)blockIdx.x * 768, blockIdx.y * PER, blockIdx.y * PER + PER);
}

// ------------------------------------------------------------------------------ C ABI
// Workspace: 6 time rows (6 x 768 fp32) | per-workgroup error partials (fp64).
size_t ode_part_offset() { return 6 * 768 * sizeof(float); }

extern "C" size_t gp_ode_workspace_size(int rows) {
    return ode_part_offset() + sizeof(double) * (((size_t)rows + 15) / 16) + 256;
}

int ode_launch_times(const gp_head_weights* w, const float* t32, int nt, void* ws, hipStream_t stream) {
    OdeTimes tv = {};
    for (int i = 0; i < nt; ++i) tv.t[i] = t32[i];
    hipLaunchKernelGGL(ode_time_rows_kernel, dim3(nt, ODE_ROW_CHUNKS), dim3(HT), 0, stream, *w, tv,
                       static_cast<float*>(ws));
    return gp_check_launch("ode_time_rows_kernel");
}

int ode_launch_norm(const double* part, int n, double count, double* out, hipStream_t stream) {
    hipLaunchKernelGGL(ode_norm_kernel, dim3(1), dim3(256), 0, stream, part, n, count, out);
    return gp_check_launch("ode_norm_kernel");
}

extern "C" int gp_ode_rhs(const gp_head_weights* w, const float* pobj, float t32, float sigma, double coef,
                          const double* y, const double* const* kin, const double* acoef, int nk, double h, int rows,
                          int k, double* kout, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    return ode_rhs_once("ode_rhs", w, pobj, t32, sigma, coef, y, kin, acoef, nk, h, rows, k, kout, workspace,
                        workspace_bytes, stream,
                        [&](const OdeStageArgs& a) {
                            return ode_launch_stage(a, ode_nt(w, rows), false, "ode_stage_kernel", stream);
                        });
}

extern "C" int gp_ode_attempt(const gp_head_weights* w, const float* pobj, const float* t32_6, const float* sigma_6,
                              const double* coef_6, const double* y, double* const* kslots, const double* tableau_a,
                              const double* b, const double* e, double h, double rtol, double atol, int rows, int k,
                              double* ynew, double* err_out, void* workspace, size_t workspace_bytes,
                              hipStream_t stream) {
    return ode_attempt_host(
        "ode_attempt", w, pobj, t32_6, sigma_6, coef_6, y, kslots, tableau_a, b, e, h, rtol, atol, rows, k, ynew, err_out,
        workspace, workspace_bytes, stream, [&] { return ode_nwg(w, rows); }, (double)rows * 9.0,
        [&](const OdeStageArgs& a, bool last) {
            return ode_launch_stage(a, ode_nt(w, rows), last, last ? "ode_stage_kernel<final>" : nullptr, stream);
        });
}

// ------------------------------------------------------------------------------ likelihood (host-controlled)
// Workspace as the sampler's: 6 time rows | one error partial per 16 rows (an upper bound for every tiling).
extern "C" size_t gp_like_workspace_size(int rows) { return gp_ode_workspace_size(rows); }

extern "C" int gp_like_rhs(const gp_head_weights* w, const float* pobj, float t32, float sigma, double coef,
                           const double* y, const float* eps, const double* const* kin, const double* acoef, int nk,
                           double h, int rows, int k, double* kout, void* workspace, size_t workspace_bytes,
                           hipStream_t stream) {
    GP_REQUIRE(eps, "like_rhs: bad arguments");
    return ode_rhs_once("like_rhs", w, pobj, t32, sigma, coef, y, kin, acoef, nk, h, rows, k, kout, workspace,
                        workspace_bytes, stream, [&](const OdeStageArgs& a) {
                            return like_launch_stage(a, eps, like_np(w, rows), false, "like_stage_kernel", stream);
                        });
}

extern "C" int gp_like_attempt(const gp_head_weights* w, const float* pobj, const float* t32_6, const float* sigma_6,
                               const double* coef_6, const double* y, const float* eps, double* const* kslots,
                               const double* tableau_a, const double* b, const double* e, double h, double rtol,
                               double atol, int rows, int k, double* ynew, double* err_out, void* workspace,
                               size_t workspace_bytes, hipStream_t stream) {
    GP_REQUIRE(eps, "like_attempt: bad arguments");
    return ode_attempt_host(
        "like_attempt", w, pobj, t32_6, sigma_6, coef_6, y, kslots, tableau_a, b, e, h, rtol, atol, rows, k, ynew,
        err_out, workspace, workspace_bytes, stream,
        [&] { return (rows + 16 * like_np(w, rows) - 1) / (16 * like_np(w, rows)); }, (double)rows * 10.0,
        [&](const OdeStageArgs& a, bool last) {
            return like_launch_stage(a, eps, like_np(w, rows), last, last ? "like_stage_kernel<final>" : nullptr, stream);
        });
}

extern "C" int gp_ode_init_norms(const double* y0, const double* f0, const double* f1, long long n, double atol,
                                 double rtol, double* out, hipStream_t stream) {
    GP_REQUIRE(y0 && f0 && out && n >= 1, "ode_init_norms: bad arguments");
    hipLaunchKernelGGL(ode_init_norms_kernel, dim3(1), dim3(1024), 0, stream, y0, f0, f1, n, atol, rtol, out);
    return gp_check_launch("ode_init_norms_kernel");
}

extern "C" int gp_ode_dense(const double* const* kslots, const double* P7x4, const double* y_old,
                            const double* t_eval, int i0, int i1, int i_base, int reverse, double t_old, double h,
                            long long n, double* out, hipStream_t stream) {
    GP_REQUIRE(kslots && P7x4 && y_old && t_eval && out && n >= 1 && i1 >= i0, "ode_dense: bad arguments");
    if (i1 == i0) return GP_OK;
    OdeDenseArgs a = {};
    for (int j = 0; j < ODE_NK; ++j) {
        GP_REQUIRE(kslots[j] != nullptr, "ode_dense: null K slot");
        a.k[j] = kslots[j];
        for (int m = 0; m < 4; ++m) a.P[j][m] = P7x4[j * 4 + m];
    }
    a.y_old = y_old;
    a.tev = t_eval;
    a.i0 = i0;
    a.i1 = i1;
    a.i_base = i_base;
    a.reverse = reverse;
    a.t_old = t_old;
    a.h = h;
    a.out = out;
    a.n = n;
    hipLaunchKernelGGL(ode_dense_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
    return gp_check_launch("ode_dense_kernel");
}

int ode_denoise_begin(const char* who, const gp_head_weights* w, const float* pobj, float t32, float sigma, float g2,
                      float step, const double* x, int rows, int k, const float* pts_center, double* pose, double* q,
                      void* workspace, size_t workspace_bytes, hipStream_t stream, OdeDenoiseArgs* a) {
    GP_REQUIRE(w && pobj && x && pts_center && pose && q && workspace && rows >= 1 && k >= 1, "%s: bad arguments", who);
    GP_REQUIRE(workspace_bytes >= gp_ode_workspace_size(rows), "%s: workspace too small", who);
    GP_TRY(ode_launch_times(w, &t32, 1, workspace, stream));
    *a = OdeDenoiseArgs{};
    a->w = *w;
    a->pobj = pobj;
    a->tproj = static_cast<const float*>(workspace);
    a->sigma = sigma;
    a->g2 = g2;
    a->step = step;
    a->x = x;
    a->center = pts_center;
    a->pose = pose;
    a->q = q;
    a->rows = rows;
    a->kper = k;
    return GP_OK;
}

// nt_rows: the row count that picks the tile class (rows; the whole batch's rows for a per-object slice)
static int ode_denoise_impl(const gp_head_weights* w, const float* pobj, const OdeDenoiseScalars& sc, const double* x,
                            int rows, int k, int nt_rows, const float* pts_center, double* pose, double* q,
                            void* workspace, size_t workspace_bytes, hipStream_t stream) {
    OdeDenoiseArgs a;
    GP_TRY(ode_denoise_begin("ode_denoise", w, pobj, sc.te, sc.sig, sc.g2, sc.step, x, rows, k, pts_center, pose, q,
                             workspace, workspace_bytes, stream, &a));
    // the stage kernels' trunk and tile (exact fp32 without the f16 planes)
    const int nt = ode_nt(w, nt_rows);
    const dim3 grid((rows + 16 * nt - 1) / (16 * nt)), blk(EVAL_WV * 64);
    head_dispatch(w->pe2_h ? X3P : 0, nt, [&](auto pl, auto ntc) {
        hipLaunchKernelGGL((ode_denoise_kernel<pl.value, ntc.value>), grid, blk, 0, stream, a);
    });
    return gp_check_launch("ode_denoise_kernel");
}

extern "C" int gp_ode_denoise(const gp_head_weights* w, const float* pobj, float t32, float sigma, float g2,
                              float step, const double* x, int rows, int k, const float* pts_center, double* pose,
                              double* q, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    return ode_denoise_impl(w, pobj, {t32, sigma, g2, step}, x, rows, k, rows, pts_center, pose, q, workspace,
                            workspace_bytes, stream);
}

// ============================================================================ device-controlled RK45
// The host-controlled path above reads one error norm per attempt (a device->host round trip per
// attempt, ~30% of the sampler's wall time at config 2). Here the step controller itself runs on
// the device: ode_control_kernel of attempt n decides attempt n-1 (scipy _step_impl's
// accept/reject and step-size update from its error norm) and prepares attempt n (min_step check,
// h, t_new, the 6 stage times and their scalars, and their time rows), so the host only enqueues
// attempts one ahead and reads a status word. Stage scalars use device pow(); the host path uses
// glibc's through torch: the two can differ in the last bit (tests/test_gpu_parity.py compares
// the two paths).
#define ODE_CTL_CHUNKS 8   // workgroups per stage time row (768 / 8 outputs each)

// hstat (optional, host-mapped memory): word n & 3 receives 4 n + (status + 1) once attempt n is decided and prepared,
// so a host can follow the solve without an event and a copy between the control and the stage launches
__global__ __launch_bounds__(HT) void ode_control_kernel(gp_head_weights w, const OdeCtl* __restrict__ cin,
                                                         OdeCtl* __restrict__ cout, const double* __restrict__ part,
                                                         int decide, OdeConsts k, float* __restrict__ tproj6,
                                                         int* __restrict__ hstat, int n) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    __shared__ OdeCtl s;
    __shared__ float emb[128], tf[128];
    const int tid = threadIdx.x;
    // error norm of attempt n-1 (the same fixed order in every workgroup)
    const double esum = decide ? block_sum_f64(part, k.nwg, red) : 0.0;
    if (tid == 0) {
        OdeCtl c = *cin;
        const double dir = k.direction;
        if (decide && c.active) {   // scipy RK45._step_impl, after rk_step / _estimate_error_norm
            const double err = sqrt(esum) / sqrt(k.count);
            c.nfev += 6;
            if (err < 1.0) {
                double factor = err == 0.0 ? 10.0 : fmin(10.0, 0.9 * pow(err, -0.2));
                if (c.rejected) factor = fmin(1.0, factor);
                c.h_abs = c.h_abs_loc * factor;
                c.t_old = c.t;
                c.h_last = c.h;
                c.t = c.t_new;
                c.yi ^= 1;
                const int k0 = c.kidx[0];
                c.kidx[0] = c.kidx[ODE_NK - 1];
                c.kidx[ODE_NK - 1] = k0;
                c.n_acc += 1;
                c.rejected = 0;
                if (dir * (c.t - k.t_bound) >= 0.0) c.status = 1;
            } else {
                c.h_abs_loc *= fmax(0.2, 0.9 * pow(err, -0.2));
                c.rejected = 1;
            }
        }
        c.active = 0;
        if (c.status == 0) {   // prepare the next attempt
            const double min_step = 10.0 * fabs(nextafter(c.t, dir * INFINITY) - c.t);
            double ha = c.rejected ? c.h_abs_loc : (c.h_abs < min_step ? min_step : c.h_abs);
            if (ha < min_step) {
                c.status = -1;
            } else {
                double h = ha * dir;
                double t_new = c.t + h;
                if (dir * (t_new - k.t_bound) > 0.0) t_new = k.t_bound;
                h = t_new - c.t;
                c.h = h;
                c.t_new = t_new;
                c.h_abs_loc = fabs(h);
                c.active = 1;
            }
        }
        s = c;
    }
    __syncthreads();
    if (!s.active) {
        if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) {
            *cout = s;
            if (hstat != nullptr) {
                __threadfence_system();
                reinterpret_cast<volatile int*>(hstat)[n & 3] = 4 * n + s.status + 1;
            }
        }
        return;
    }
    // stage times t + c_s h (s = 1..5) and t + h, one thread each (rk.py rk_step)
    if (tid < 6) {
        const double cs[5] = {1.0 / 5.0, 3.0 / 10.0, 4.0 / 5.0, 8.0 / 9.0, 1.0};
        const double ts = tid < 5 ? s.t + cs[tid] * s.h : s.t + s.h;
        const float t32 = (float)ts;
        s.t32[tid] = t32;
        s.sig[tid] = fmul((float)k.sig_min, (float)pow(k.base, (double)t32));
        const double g = (k.sig_min * pow(k.base, ts)) * k.diff_scale;
        s.coef[tid] = -(0.5 * (g * g));
    }
    __syncthreads();
    if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) {
        *cout = s;
        if (hstat != nullptr) {
            __threadfence_system();
            reinterpret_cast<volatile int*>(hstat)[n & 3] = 4 * n + s.status + 1;
        }
    }
    // time row slice of stage blockIdx.x: outputs [chunk * 96, chunk * 96 + 96)
    constexpr int PER = 768 / ODE_CTL_CHUNKS;
    time_row(w, s.t32[blockIdx.x], emb, tf, tproj6 + (size_t)blockIdx.x * 768, blockIdx.y * PER, blockIdx.y * PER + PER);
}

// Device-controlled attempts as one fused launch (default) or six stage launches (GENPOSE2_ODE_FUSED=0: the
// same bits; for A/B and the equality test).
static bool ode_fused() {
    const char* v = getenv("GENPOSE2_ODE_FUSED");
    return v == nullptr || v[0] != '0';
}

// Workspace of the device-controlled path: ctl[2] | time rows (6 x 768 fp32) | error partials.
static size_t auto_tproj_off() { return 2 * sizeof(OdeCtl); }
static size_t auto_part_off() { return auto_tproj_off() + 6 * 768 * sizeof(float); }

extern "C" size_t gp_ode_ctl_size(void) { return sizeof(OdeCtl); }

extern "C" size_t gp_ode_auto_workspace_size(int rows) {
    return auto_part_off() + sizeof(double) * (((size_t)rows + 15) / 16) + 256;
}

// A global-batch shard of one RK45 solve on the whole batch: the tiling of the single call (nt from rows_total), this
// shard's partials at part_off of part_n, the error norm over every shard's partials and rows_total * 9 elements,
// and after each attempt an exchange that brings every shard's partials to every rank before the next control.
struct OdeGlobal {
    int rows_total, part_n, part_off;
    gp_ode_exchange_fn exchange;
    void* ctx;
};

static size_t ode_auto_ws_bytes(int part_n) { return auto_part_off() + sizeof(double) * (size_t)part_n + 256; }

// What every gp_ode_auto_attempt* entry hands on as it got it, in the entries' order
struct OdeAutoParams {
    const gp_head_weights* w;
    const float* pobj;
    int n, what;
    double t_bound, direction, rtol, atol, sig_min, base, diff_scale;
    double *y0, *y1;
    double* const* kslots;
    const double *tableau_a, *b, *e;
    int rows, k;
    void* workspace;
    size_t workspace_bytes;
    hipStream_t stream;
};

// g: a global-batch shard, or null; hstat: the host-mapped status words, or null; gw: the energy agent's
// transposed weights, or null for the score agent
static int ode_auto_attempt_impl(const OdeAutoParams& p, const OdeGlobal* g, int* hstat,
                                 const gp_head_grad_weights* gw) {
    GP_REQUIRE(p.w && p.pobj && p.y0 && p.y1 && p.kslots && p.tableau_a && p.b && p.e && p.workspace && p.rows >= 1 &&
                   p.k >= 1 && p.n >= 0,
               "ode_auto_attempt: bad arguments");
    for (int j = 0; j < ODE_NK; ++j) GP_REQUIRE(p.kslots[j] != nullptr, "ode_auto_attempt: null K slot");
    const int n = p.n, rows = p.rows;
    const hipStream_t stream = p.stream;
    char* ws = static_cast<char*>(p.workspace);
    OdeCtl* ctl = reinterpret_cast<OdeCtl*>(ws);
    float* tproj6 = reinterpret_cast<float*>(ws + auto_tproj_off());
    double* part = reinterpret_cast<double*>(ws + auto_part_off());
    // gw: the energy agent's stages (gp_ode_energy.hip), 16-row tiles whatever the trunk arithmetic of w
    const int nt = gw ? 1 : ode_nt(p.w, g ? g->rows_total : rows);
    const int nwg = (rows + 16 * nt - 1) / (16 * nt);   // this call's workgroups
    const int part_n = g ? g->part_n : nwg;
    GP_REQUIRE(!g || (g->part_off >= 0 && g->part_off + nwg <= part_n),
               "ode_auto_attempt: shard partials [%d, %d) outside %d", g ? g->part_off : 0, g ? g->part_off + nwg : 0,
               part_n);
    GP_REQUIRE(p.workspace_bytes >= ode_auto_ws_bytes(part_n), "ode_auto_attempt: workspace too small");
    OdeConsts kc = {p.t_bound, p.direction, p.rtol, p.atol, p.sig_min, p.base, p.diff_scale,
                    (double)(g ? g->rows_total : rows) * 9.0, part_n};
    OdeCtl* cin = ctl + (n & 1);
    OdeCtl* cout = ctl + ((n + 1) & 1);
    GP_REQUIRE(p.what >= 1 && p.what <= 3, "ode_auto_attempt: what must be 1 (control), 2 (stages) or 3 (both)");
    if (p.what & 1) {
        hipLaunchKernelGGL(ode_control_kernel, dim3(6, ODE_CTL_CHUNKS), dim3(HT), 0, stream, *p.w, (const OdeCtl*)cin,
                           cout, (const double*)part, n > 0 ? 1 : 0, kc, tproj6, hstat, n);
        const int rc = gp_check_launch("ode_control_kernel");
        if (rc || !(p.what & 2)) return rc;
    }
    OdeStageArgs a = {};
    a.w = *p.w;
    a.pobj = p.pobj;
    a.rows = rows;
    a.kper = p.k;
    a.part_off = g ? g->part_off : 0;
    a.rtol = p.rtol;
    a.atol = p.atol;
    a.ctl = cout;
    a.tproj6 = tproj6;
    a.ybuf[0] = p.y0;
    a.ybuf[1] = p.y1;
    for (int j = 0; j < ODE_NK; ++j) a.kbuf[j] = p.kslots[j];
    int rc;
    if (ode_fused()) {   // one launch per attempt (ode_attempt_kernel)
        const OdeTableau tb = ode_tableau(p.tableau_a, p.b);
        for (int j = 0; j < ODE_NK; ++j) a.e[j] = p.e[j];
        a.part = part;
        if (gw) return ode_energy_launch_attempt(a, *gw, tb, stream);
        const dim3 grid(nwg), blk(EVAL_WV * 64);
        head_dispatch(p.w->pe2_h ? X3P : 0, nt, [&](auto pl, auto ntc) {
            hipLaunchKernelGGL((ode_attempt_kernel<pl.value, ntc.value>), grid, blk, 0, stream, a, tb);
        });
        rc = gp_check_launch("ode_attempt_kernel");
    } else {   // the six stage launches, their scalars from the controller's record
        rc = ode_run_stages(
            a, p.tableau_a, p.b, p.e, nullptr, part, [](OdeStageArgs& s, int st) { s.stage = st; },
            [&](const OdeStageArgs& s, bool last) {
                return gw ? ode_energy_launch_stage(s, *gw, last, stream)
                          : ode_launch_stage(s, nt, last, last ? "ode_stage_kernel<auto>" : nullptr, stream);
            });
    }
    if (rc || !g) return rc;
    GP_REQUIRE(g->exchange(g->ctx, n, part, part_n, stream) == 0, "ode_auto_attempt: partials exchange of attempt %d", n);
    return GP_OK;
}

extern "C" int gp_ode_auto_attempt(const gp_head_weights* w, const float* pobj, int n, int what,
                                   double t_bound, double direction, double rtol, double atol, double sig_min,
                                   double base, double diff_scale, double* y0, double* y1,
                                   double* const* kslots, const double* tableau_a, const double* b,
                                   const double* e, int rows, int k, void* workspace, size_t workspace_bytes,
                                   hipStream_t stream) {
    return ode_auto_attempt_impl({w, pobj, n, what, t_bound, direction, rtol, atol, sig_min, base, diff_scale, y0, y1,
                                  kslots, tableau_a, b, e, rows, k, workspace, workspace_bytes, stream},
                                 nullptr, nullptr, nullptr);
}

extern "C" int gp_ode_auto_attempt_hs(const gp_head_weights* w, const float* pobj, int n, int what,
                                      double t_bound, double direction, double rtol, double atol, double sig_min,
                                      double base, double diff_scale, double* y0, double* y1,
                                      double* const* kslots, const double* tableau_a, const double* b,
                                      const double* e, int rows, int k, void* workspace, size_t workspace_bytes,
                                      int* host_status, hipStream_t stream) {
    GP_REQUIRE(host_status != nullptr, "ode_auto_attempt_hs: null status words");
    return ode_auto_attempt_impl({w, pobj, n, what, t_bound, direction, rtol, atol, sig_min, base, diff_scale, y0, y1,
                                  kslots, tableau_a, b, e, rows, k, workspace, workspace_bytes, stream},
                                 nullptr, host_status, nullptr);
}

extern "C" int gp_ode_auto_attempt_energy(const gp_head_weights* w, const gp_head_grad_weights* gw, const float* pobj,
                                          int n, int what, double t_bound, double direction, double rtol,
                                          double atol, double sig_min, double base, double diff_scale, double* y0,
                                          double* y1, double* const* kslots, const double* tableau_a,
                                          const double* b, const double* e, int rows, int k, void* workspace,
                                          size_t workspace_bytes, int* host_status, hipStream_t stream) {
    GP_REQUIRE(ode_energy_weights_ok(gw), "ode_auto_attempt_energy: null transposed weights");
    return ode_auto_attempt_impl({w, pobj, n, what, t_bound, direction, rtol, atol, sig_min, base, diff_scale, y0, y1,
                                  kslots, tableau_a, b, e, rows, k, workspace, workspace_bytes, stream},
                                 nullptr, host_status, gw);
}

extern "C" int gp_ode_global_partials(int rows_total, int shard_rows_max, int shards, int split) {
    if (rows_total < 1 || shard_rows_max < 1 || shards < 1) return 0;
    const int tile = 16 * head_pick_nt(rows_total, split != 0);
    return shards * ((shard_rows_max + tile - 1) / tile);
}

extern "C" size_t gp_ode_global_workspace_size(int part_n) { return part_n >= 1 ? ode_auto_ws_bytes(part_n) : 0; }

extern "C" size_t gp_ode_auto_partials_offset(void) { return auto_part_off(); }

extern "C" int gp_ode_auto_attempt_global(const gp_head_weights* w, const float* pobj, int n, int what,
                                          double t_bound, double direction, double rtol, double atol, double sig_min,
                                          double base, double diff_scale, double* y0, double* y1,
                                          double* const* kslots, const double* tableau_a, const double* b,
                                          const double* e, int rows, int k, int rows_total, int row_off, int shard,
                                          int shards, int shard_rows_max, gp_ode_exchange_fn exchange, void* ctx,
                                          void* workspace, size_t workspace_bytes, int* host_status,
                                          hipStream_t stream) {
    GP_REQUIRE(w && exchange, "ode_auto_attempt_global: null pointer");
    GP_REQUIRE(shards >= 1 && shard >= 0 && shard < shards && rows >= 1 && rows <= shard_rows_max && row_off >= 0 &&
                   row_off + rows <= rows_total,
               "ode_auto_attempt_global: shard %d of %d, rows [%d, %d) of %d (at most %d per shard)", shard, shards,
               row_off, row_off + rows, rows_total, shard_rows_max);
    const int tile = 16 * ode_nt(w, rows_total);
    const int per = (shard_rows_max + tile - 1) / tile;
    OdeGlobal g = {rows_total, shards * per, shard * per, exchange, ctx};
    return ode_auto_attempt_impl({w, pobj, n, what, t_bound, direction, rtol, atol, sig_min, base, diff_scale, y0, y1,
                                  kslots, tableau_a, b, e, rows, k, workspace, workspace_bytes, stream},
                                 &g, host_status, nullptr);
}

// ============================================================================ whole sampler (C hosts)
// cond_ode_sampler (samplers.py:180-258) in one call for hosts without Python: select_initial_step
// (scipy _ivp/common.py) from two host-scalar RHS evaluations, then the device-controlled attempts
// (gp_ode_auto_attempt) kept one attempt ahead of a 4-byte status read, the dense output at eps when
// `steps` > 0 (t_eval = linspace(T0, eps, steps): only its last point reaches cond_ode_sampler), the
// final denoise step and the epilogue (gp_ode_denoise). genpose2_amd/ode.py (rk45_device) and
// agent.py (PoseNet._ode) are the Python form of the same sequence.
namespace {
struct OdeSampleLayout {
    OdeStateBlock st;   // y and ynew: the two state buffers of the device controller
    size_t dense, scal, rhs_ws, auto_ws, total;
};
OdeSampleLayout ode_sample_layout(int rows) {
    OdeSampleLayout L = {};
    size_t off = 0;
    L.st = ode_state_layout(off, rows, 9);
    L.dense = off; off += align256((size_t)rows * 9 * sizeof(double));
    L.scal = off; off += 256;
    L.rhs_ws = off; off += align256(gp_ode_workspace_size(rows));
    L.auto_ws = off; off += align256(gp_ode_auto_workspace_size(rows));
    L.total = off;
    return L;
}
}  // namespace

std::mutex g_status_mu;
std::vector<StatusReader> g_status_pool;

__global__ void f32_to_f64_kernel(const float* __restrict__ in, double* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (double)in[i];
}

extern "C" size_t gp_ode_sample_workspace_size(int rows) { return rows >= 1 ? ode_sample_layout(rows).total : 0; }

// The attempts of a whole solve, one enqueued ahead of the status read, for every whole-solve entry. launch(n, what)
// enqueues attempt n's control (what & 1: decides attempt n - 1, prepares n, writes its status word) and its stages
// (what & 2: a no-op once the solve has ended). hs_dev (StatusLease::map) non-null: the control of attempt n writes
// 4 n + state (state 1: running) into pinned word n & 3 and the host polls it; nothing sits between a control launch
// and its stage launch. Null: the 4-byte word at stat_src(n) is copied behind control n, with an event, ahead of
// attempt n's stages; `numbered`: that word is 4 n + state too, else it is nonzero once the solve has ended.
// *last + 1 is the attempt whose control saw the end: the final records are those of parity (*last + 2) & 1.
template <typename Launch, typename Src>
static int ode_run_attempts(StatusLease& status, const int* hs_dev, bool numbered, Launch launch, Src stat_src,
                            const char* who, int* last) {
    int rc, a = 0;
    if (hs_dev != nullptr) status.pending = true;   // the device writes the words until the stream drains
    if ((rc = launch(0, 3))) return rc;
    for (;; ++a) {
        GP_REQUIRE(a < 100000, "%s: attempt limit reached", who);
        const int want = a + 1;   // its control decides attempt a
        int v;
        if (hs_dev != nullptr) {
            if ((rc = launch(want, 3))) return rc;
            volatile int* hv = status.r.pinned;
            const auto t_end = std::chrono::steady_clock::now() + std::chrono::seconds(60);
            while (((v = hv[want & 3]) >> 2) != want)
                GP_REQUIRE(std::chrono::steady_clock::now() < t_end, "%s: no status from attempt %d", who, want);
            if ((v & 3) != 1) break;
        } else {
            if ((rc = launch(want, 1))) return rc;
            status.pending = true;
            GP_REQUIRE(hipMemcpyAsync(status.r.pinned, stat_src(want), 4, hipMemcpyDeviceToHost, status.stream) ==
                               hipSuccess && hipEventRecord(status.r.ev, status.stream) == hipSuccess,
                       "%s: status read", who);
            if ((rc = launch(want, 2))) return rc;
            GP_REQUIRE(hipEventSynchronize(status.r.ev) == hipSuccess, "%s: status wait", who);
            status.pending = false;
            v = *status.r.pinned;
            GP_REQUIRE(!numbered || (v >> 2) == want, "%s: status word of attempt %d", who, want);
            if (numbered ? (v & 3) != 1 : v != 0) break;
        }
    }
    *last = a;
    return GP_OK;
}

// gw: null for the score agent; the energy agent's transposed weights otherwise (its right-hand sides, attempts
// and denoise are gp_ode_rhs_energy, gp_ode_auto_attempt_energy and gp_ode_denoise_energy)
static int ode_sample_impl(const gp_head_weights* w, const gp_head_grad_weights* gw, const float* pobj,
                           const float* x0, int rows, int k, double T0, double eps, int steps, double rtol,
                           double atol, const float* pts_center, double* pose, double* q, int* nfev_out,
                           int* status_out, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    GP_REQUIRE(w && pobj && x0 && pts_center && pose && q && workspace && rows >= 1 && k >= 1 && steps >= 0,
               "ode_sample: bad arguments");
    GP_REQUIRE(T0 != eps, "ode_sample: empty integration interval (T0 == eps)");
    GP_REQUIRE(steps != 1, "ode_sample: steps must be 0 (t_eval unset) or >= 2");
    const OdeSampleLayout L = ode_sample_layout(rows);
    GP_REQUIRE(workspace_bytes >= L.total, "ode_sample: workspace too small (gp_ode_sample_workspace_size)");
    StatusLease status;
    GP_REQUIRE(status.acquire(stream) == 0, "ode_sample: pinned status word / event");
    char* ws = static_cast<char*>(workspace);
    double* y[2] = {reinterpret_cast<double*>(ws + L.st.y), reinterpret_cast<double*>(ws + L.st.ynew)};
    double* K[ODE_NK];
    for (int j = 0; j < ODE_NK; ++j) K[j] = reinterpret_cast<double*>(ws + L.st.k[j]);
    double* f1 = reinterpret_cast<double*>(ws + L.st.f1);
    double* dense = reinterpret_cast<double*>(ws + L.dense);
    double* scal = reinterpret_cast<double*>(ws + L.scal);
    void* rws = ws + L.rhs_ws;
    void* aws = ws + L.auto_ws;
    const size_t rws_b = gp_ode_workspace_size(rows), aws_b = gp_ode_auto_workspace_size(rows);
    const long long n = (long long)rows * 9;
    const double t0 = T0, tf = eps, dir = tf > t0 ? 1.0 : -1.0;
    const double dscale = diff_scale();
    int rc;
    auto rhs = [&](float t32, double coef, const double* const* kin, const double* acoef, int nk, double h,
                   double* kout) {
        return gw ? gp_ode_rhs_energy(w, gw, pobj, t32, sigma32(t32), coef, y[0], kin, acoef, nk, h, rows, k, kout,
                                      rws, rws_b, stream)
                  : gp_ode_rhs(w, pobj, t32, sigma32(t32), coef, y[0], kin, acoef, nk, h, rows, k, kout, rws, rws_b,
                               stream);
    };
    hipLaunchKernelGGL(f32_to_f64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x0, y[0], n);
    if ((rc = gp_check_launch("f32_to_f64_kernel"))) return rc;

    // ---- select_initial_step (scipy common.py), as genpose2_amd/ode.py initial_step
    {   // f(t0)
        const float t32 = (float)t0;
        if ((rc = rhs(t32, ode_coef_t0(t32, dscale), nullptr, nullptr, 0, 0.0, K[0]))) return rc;
    }
    if ((rc = gp_ode_init_norms(y[0], K[0], nullptr, n, atol, rtol, scal, stream))) return rc;
    double hs[3];
    GP_TRY(ode_copy_sync(hs, scal, 2 * sizeof(double), hipMemcpyDeviceToHost, stream, "ode_sample", "norm read"));
    const double interval = fabs(tf - t0);
    const double h0 = ode_init_h0(hs[0], hs[1], interval);
    {   // f(t0 + h0 dir, y0 + h0 dir f0)
        const double t = t0 + h0 * dir;
        const double a1 = 1.0;
        const double* kin[1] = {K[0]};
        if ((rc = rhs((float)t, ode_coef(t, dscale), kin, &a1, 1, h0 * dir, f1))) return rc;
    }
    if ((rc = gp_ode_init_norms(y[0], K[0], f1, n, atol, rtol, scal, stream))) return rc;
    GP_TRY(ode_copy_sync(hs + 2, scal + 2, sizeof(double), hipMemcpyDeviceToHost, stream, "ode_sample", "norm read"));

    // ---- device-controlled attempts, one enqueued ahead of the status read
    OdeCtl c0 = {};
    c0.t = t0;
    c0.h_abs = ode_init_h_abs(h0, hs[1], hs[2], interval);
    c0.nfev = 2;
    for (int j = 0; j < ODE_NK; ++j) c0.kidx[j] = j;
    GP_TRY(ode_copy_sync(aws, &c0, sizeof(OdeCtl), hipMemcpyHostToDevice, stream, "ode_sample", "controller record"));
    const char* ctl = static_cast<const char*>(aws);   // OdeCtl[2]; attempt n's control writes parity (n + 1) & 1
    int* hs_dev = status.map(false);
    auto launch = [&](int n, int what) {
        return ode_auto_attempt_impl({w, pobj, n, what, tf, dir, rtol, atol, kSigMin, kBase, dscale, y[0], y[1], K, kA6,
                                      kB6, kE7, rows, k, aws, aws_b, stream},
                                     nullptr, hs_dev, gw);
    };
    auto stat_src = [&](int n) { return ctl + ((n + 1) & 1) * sizeof(OdeCtl) + offsetof(OdeCtl, status); };
    int a = 0;
    if ((rc = ode_run_attempts(status, hs_dev, false, launch, stat_src, "ode_sample", &a))) return rc;
    OdeCtl c;
    GP_TRY(ode_copy_sync(&c, ctl + ((a + 2) & 1) * sizeof(OdeCtl), sizeof(OdeCtl), hipMemcpyDeviceToHost, stream,
                         "ode_sample", "final record"));
    status.pending = false;
    if (status_out) *status_out = c.status;
    if (nfev_out) *nfev_out = c.nfev;
    GP_REQUIRE(!(c.status < 0 && steps > 0),
               "ode_sample: RK45 failed (step size below the spacing of t) with t_eval set: the collected t_eval "
               "outputs need the host controller (genpose2_amd/ode.py rk45_drive)");
    const double* x = y[c.yi];
    if (steps > 0 && c.status > 0) {   // res.y[:, -1]: the final step's dense output at t_eval[-1] = eps
        const double* ks[ODE_NK];
        for (int j = 0; j < ODE_NK; ++j) ks[j] = K[c.kidx[j]];
        std::swap(ks[0], ks[ODE_NK - 1]);   // undo the FSAL swap of the accepted step
        GP_TRY(ode_copy_sync(scal + 7, &eps, sizeof(double), hipMemcpyHostToDevice, stream, "ode_sample", "t_eval"));
        if ((rc = gp_ode_dense(ks, kP74, y[c.yi ^ 1], scal + 7, 0, 1, 0, 0, c.t_old, c.t - c.t_old, n, dense, stream)))
            return rc;
        x = dense;
    }
    // ---- denoise (samplers.py:240-249) with eps's scalars
    const OdeDenoiseScalars ds = ode_denoise_scalars(eps, steps);
    if (gw)
        return gp_ode_denoise_energy(w, gw, pobj, ds.te, ds.sig, ds.g2, ds.step, x, rows, k, pts_center, pose, q, rws,
                                     rws_b, stream);
    return gp_ode_denoise(w, pobj, ds.te, ds.sig, ds.g2, ds.step, x, rows, k, pts_center, pose, q, rws, rws_b, stream);
}

extern "C" int gp_ode_sample(const gp_head_weights* w, const float* pobj, const float* x0, int rows, int k, double T0,
                             double eps, int steps, double rtol, double atol, const float* pts_center, double* pose,
                             double* q, int* nfev_out, int* status_out, void* workspace, size_t workspace_bytes,
                             hipStream_t stream) {
    return ode_sample_impl(w, nullptr, pobj, x0, rows, k, T0, eps, steps, rtol, atol, pts_center, pose, q, nfev_out,
                           status_out, workspace, workspace_bytes, stream);
}

extern "C" int gp_ode_sample_energy(const gp_head_weights* w, const gp_head_grad_weights* gw, const float* pobj,
                                    const float* x0, int rows, int k, double T0, double eps, int steps, double rtol,
                                    double atol, const float* pts_center, double* pose, double* q, int* nfev_out,
                                    int* status_out, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    GP_REQUIRE(ode_energy_weights_ok(gw), "ode_sample_energy: null transposed weights");
    return ode_sample_impl(w, gw, pobj, x0, rows, k, T0, eps, steps, rtol, atol, pts_center, pose, q, nfev_out,
                           status_out, workspace, workspace_bytes, stream);
}

// ============================================================================ per-object RK45 (gp_ode_sample_object)
// cond_ode_sampler as the reference runs it when called once per object on that object's k candidates: every
// object has its own solve_ivp -- its own initial step, step controller, stage times, accept / reject and RMS
// norms over its k * 9 elements -- so its result does not depend on which other objects share the call.
//
// One OdeObjRec per object, double-buffered per attempt parity as OdeCtl is. ode_obj_control_kernel (one workgroup
// per object and slice of the 768-row) decides the object's last attempt from its rows' error sums and prepares
// the next one: h, t_new, the six stage scalars, and the six rows init[s][b] = pobj[b] + tproj(t32[b][s]) (one fp32
// add, the sum the trunks form themselves from pobj and tproj). The stages hand the trunk init[s] as its pobj and a
// row of -0.0f as its tproj: x + (-0.0f) is x for every x, so a row's bits are those of the whole-batch stage at
// the same t32 and the trunks stay as they are. ode_obj_attempt_kernel runs the six stages of every object's
// attempt in one launch with the tiling of the whole batch (rows_total): h, coef, sigma and active / inactive are
// per row, from the row's object record; a workgroup without an active row returns at once. The K slots and the
// two state buffers keep their places: the workgroup that owns an accepted object's rows copies y_new -> y and
// K_6 -> K_0 (FSAL) in the next attempt's prologue, and only when that object runs again, so a finished object's
// y (the last step's start), y_new (its end) and K_0..K_6 stay for the dense output and are never written again.
struct OdeObjArgs {
    gp_head_weights w;
    const float* init;            // (6, nobj, 768) folded rows of the prepared attempt
    const float* zrow;            // (768) of -0.0f
    const OdeObjRec* rec;         // (nobj) records of the prepared attempt
    double* y;                    // (R,9) state at the step's start
    double* ynew;                 // (R,9) the attempt's end
    double* k[ODE_NK];            // K_0..K_6, fixed slots
    double* f1;                   // (R,9) the Euler probe's derivative (select_initial_step)
    double* rowsq;                // (R) sum over a row's 9 entries of (err/scale)^2, in increasing entry order
    double e[ODE_NK];
    double rtol, atol;
    int rows, kper, nobj;
    int single;                   // 0: an attempt; 1: K_0 = f(t, y); 2: f1 = f(t, y + K_0 h) (both with slot 0's row)
};

// ode_stage_body with h, coef, sigma and active / inactive per row (rh, rcoef, rsig, ract: LDS, one per row of the
// tile; rh and ract set before the caller's last barrier). slot: which of the attempt's six rows and scalars.
template <int MODE, int PL, int NT>
__device__ __forceinline__ void ode_obj_stage_body(const OdeObjArgs& a, const double* const* kin, const double* acoef,
                                                   int nk, int slot, double* kout, HeadSmem<NT, EVAL_WV, PL>& sm,
                                                   const int* obj, const int* ract, const double* rh, double* rcoef,
                                                   float* rsig, double* y0s, double* y1s, const SplitScalars& hs) {
    constexpr int ROWS = 16 * NT;
    constexpr int NTH = EVAL_WV * 64;
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * ROWS;
    stage_small_weights(a.w, sm);
    for (int i = tid; i < ROWS * 16; i += NTH) {
        const int c = i >> 4, j = i & 15;
        const int r = r0 + c;
        float xv = 0.f;
        if (r < a.rows && j < 9 && ract[c]) {
            const size_t e = (size_t)r * 9 + j;
            const double yv = a.y[e];
            const double yi = nk > 0 ? ode_stage_in(kin, acoef, nk, rh[c], e, yv) : yv;
            xv = (float)yi;   // torch.tensor(x, dtype=torch.float32) (samplers.py:210)
            if (MODE == 1) {
                y0s[c * 9 + j] = yv;
                y1s[c * 9 + j] = yi;
                a.ynew[e] = yi;
            }
        }
        sm.xin[i] = xv;
    }
    if (tid < ROWS) {
        const OdeObjRec* rc = a.rec + obj[tid];
        rcoef[tid] = rc->coef[slot];
        rsig[tid] = rc->sig[slot];
    }
    run_head_trunk(a.w, a.init + (size_t)slot * a.nobj * 768, a.zrow, obj, sm, 0, hs);
    for (int e9 = tid; e9 < ROWS * 9; e9 += NTH) {
#pragma clang fp contract(off)
        const int c = e9 / 9, o = e9 - c * 9;
        const int r = r0 + c;
        if (r < a.rows && ract[c]) {
            const size_t e = (size_t)r * 9 + o;
            const float s = fdiv(head_out(sm, c, o), fadd(rsig[c], 1e-7f));
            const double kv = rcoef[c] * (double)s;
            kout[e] = kv;
            if (MODE == 1) {
                const double er = ode_err_term(a, kin, kv, rh[c], e, y0s[e9], y1s[e9]);
                y1s[e9] = er * er;   // its own entry: read above by this thread only
            }
        }
    }
    if (MODE == 1) {
        __syncthreads();
        if (tid < ROWS && r0 + tid < a.rows && ract[tid]) {
#pragma clang fp contract(off)
            double sq = y1s[tid * 9];
            for (int o = 1; o < 9; ++o) sq += y1s[tid * 9 + o];
            a.rowsq[r0 + tid] = sq;
        }
    }
}

template <int PL, int NT>
__global__ __launch_bounds__(EVAL_WV * 64) void ode_obj_attempt_kernel(OdeObjArgs a, OdeTableau tb) {
    constexpr int ROWS = 16 * NT;
    constexpr int NTH = EVAL_WV * 64;
    static_assert(ROWS + 42 + ODE_NK <= NTH, "one thread per row, tableau entry and K slot");
    __shared__ HeadSmem<NT, EVAL_WV, PL> sm;
    __shared__ int obj[ROWS], ract[ROWS], rpend[ROWS];
    __shared__ double rh[ROWS], rcoef[ROWS];
    __shared__ float rsig[ROWS];
    __shared__ double y0s[ROWS * 9], y1s[ROWS * 9];
    __shared__ double tab[42];
    __shared__ const double* kin[ODE_NK];
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * ROWS;
    // none of this workgroup's objects runs: done
    if (!ode_obj_rows_to_lds<ROWS, false>(a, tb, r0, obj, ract, rpend, rh, tab, kin)) return;
    if (a.single) {
        const SplitScalars hs = load_split_scalars<PL>(a.w);
        if (a.single == 1)
            ode_obj_stage_body<0, PL, NT>(a, kin, tab, 0, 0, a.k[0], sm, obj, ract, rh, rcoef, rsig, y0s, y1s, hs);
        else   // y + (K_0 * 1.0) h
            ode_obj_stage_body<0, PL, NT>(a, kin, tab, 1, 0, a.f1, sm, obj, ract, rh, rcoef, rsig, y0s, y1s, hs);
        return;
    }
    // the accepted step of the objects that go on: y_new -> y, K_6 -> K_0 (these rows are this workgroup's in every
    // attempt; the barrier orders the stores before the stages' loads)
    for (int e9 = tid; e9 < ROWS * 9; e9 += NTH) {
        const int c = e9 / 9;
        if (ract[c] && rpend[c]) {
            const size_t e = (size_t)r0 * 9 + e9;
            a.y[e] = a.ynew[e];
            a.k[0][e] = a.k[ODE_NK - 1][e];
        }
    }
    for (int s = 1; s < 6; ++s) {
        __syncthreads();   // the copies above; stage s-1's K stores and its reads of the staged weights are done
        const SplitScalars hs = load_split_scalars<PL>(a.w);
        ode_obj_stage_body<0, PL, NT>(a, kin, tab + s * 6, s, s - 1, const_cast<double*>(kin[s]), sm, obj, ract, rh,
                                      rcoef, rsig, y0s, y1s, hs);
    }
    __syncthreads();
    const SplitScalars hs = load_split_scalars<PL>(a.w);
    ode_obj_stage_body<1, PL, NT>(a, kin, tab + 36, 6, 5, const_cast<double*>(kin[6]), sm, obj, ract, rh, rcoef, rsig,
                                  y0s, y1s, hs);
}

// dot_chains for P vectors x[p] (stride xs) against the same weight column: every weight is loaded once for the P
// sums; each sum has dot_chains' own chains and tree, so its bits.
template <int N, int CH, int P>
__device__ __forceinline__ void dot_chains_multi(const float* __restrict__ W, size_t stride, const float* x, int xs,
                                                 float (&out)[P]) {
#if HOIST64
    for (int q = 0; q < P; ++q) out[q] = (float)dot_f64<N>(W, stride, x + q * xs);
#else
    float p[P][CH];
#pragma unroll
    for (int q = 0; q < P; ++q)
#pragma unroll
        for (int j = 0; j < CH; ++j) p[q][j] = 0.f;
#pragma unroll 1   // more loads in flight (unroll 4) measured no faster: the rows are bound by the weights' L2 stream
    for (int c0 = 0; c0 < N; c0 += CH) {
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const float wv = W[(size_t)(c0 + j) * stride];
#pragma unroll
            for (int q = 0; q < P; ++q) p[q][j] = fmaf(wv, x[q * xs + c0 + j], p[q][j]);
        }
    }
#pragma unroll
    for (int q = 0; q < P; ++q) {
#pragma unroll
        for (int s = CH / 2; s >= 1; s >>= 1)
#pragma unroll
            for (int j = 0; j < s; ++j) p[q][j] += p[q][j + s];
        out[q] = p[q][0];
    }
#endif
}

#define ODE_OBJ_CHUNKS 3   // workgroups per object (768 / 3 outputs each: one per thread and stage)

// Decides attempt n-1 of object blockIdx.x (decide) and prepares its attempt n: ode_control_kernel's expressions
// on the object's own error norm. ns time rows per object (6; 1 for the two select_initial_step evaluations, whose
// records the host prepared: prepare = 0 then only forms init[0]). Every slice's workgroup of an object computes
// the same record; slice 0 writes it and counts. count: one 64-bit word, objects arrived << 32 | objects running;
// the last arriver writes 4 n + (running ? 1 : 2) to hstat[n & 3] (host-mapped, optional) and dstat[0], and zeroes
// the word for the next attempt.
__global__ __launch_bounds__(HT) void ode_obj_control_kernel(gp_head_weights w, const float* __restrict__ pobj,
                                                             const OdeObjRec* __restrict__ cin,
                                                             OdeObjRec* __restrict__ cout,
                                                             const double* __restrict__ rowsq, int decide, int prepare,
                                                             int ns, OdeConsts k, int kper, int nobj,
                                                             float* __restrict__ init,
                                                             unsigned long long* __restrict__ count,
                                                             int* __restrict__ hstat, int* __restrict__ dstat, int n) {
#pragma clang fp contract(off)
    __shared__ OdeObjRec s;
    __shared__ float emb[6 * 128], tf[6 * 128];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const bool writer = tid == 0 && blockIdx.y == 0;
    if (prepare) {
        const bool run = decide && cin[b].active;
        double esum = 0.0;
        if (run && tid < 64) {   // the object's error sum over its rows, by wave 0
            const double* rs = rowsq + (size_t)b * kper;
            esum = ode_obj_wave_sum(kper, [&](int j) { return rs[j]; });
        }
        if (tid == 0) {
            OdeObjRec c = cin[b];
            const double dir = k.direction;
            if (run) {   // scipy RK45._step_impl, after rk_step / _estimate_error_norm
                const double err = sqrt(esum) / sqrt(k.count);
                c.nfev += 6;
                c.pend = 0;
                if (err < 1.0) {
                    double factor = err == 0.0 ? 10.0 : fmin(10.0, 0.9 * pow(err, -0.2));
                    if (c.rejected) factor = fmin(1.0, factor);
                    c.h_abs = c.h_abs_loc * factor;
                    c.t_old = c.t;
                    c.t = c.t_new;
                    c.pend = 1;
                    c.n_acc += 1;
                    c.rejected = 0;
                    if (dir * (c.t - k.t_bound) >= 0.0) c.status = 1;
                } else {
                    c.h_abs_loc *= fmax(0.2, 0.9 * pow(err, -0.2));
                    c.rejected = 1;
                }
            }
            c.active = 0;
            if (c.status == 0) {   // prepare the next attempt
                const double min_step = 10.0 * fabs(nextafter(c.t, dir * INFINITY) - c.t);
                double ha = c.rejected ? c.h_abs_loc : (c.h_abs < min_step ? min_step : c.h_abs);
                if (ha < min_step) {
                    c.status = -1;
                } else {
                    double h = ha * dir;
                    double t_new = c.t + h;
                    if (dir * (t_new - k.t_bound) > 0.0) t_new = k.t_bound;
                    h = t_new - c.t;
                    c.h = h;
                    c.t_new = t_new;
                    c.h_abs_loc = fabs(h);
                    c.active = 1;
                }
            }
            s = c;
        }
        __syncthreads();
        // stage times t + c_s h (s = 1..5) and t + h, one thread each (rk.py rk_step)
        if (s.active && tid < 6) {
            const double cs[5] = {1.0 / 5.0, 3.0 / 10.0, 4.0 / 5.0, 8.0 / 9.0, 1.0};
            const double ts = tid < 5 ? s.t + cs[tid] * s.h : s.t + s.h;
            const float t32 = (float)ts;
            s.t32[tid] = t32;
            s.sig[tid] = fmul((float)k.sig_min, (float)pow(k.base, (double)t32));
            const double g = (k.sig_min * pow(k.base, ts)) * k.diff_scale;
            s.coef[tid] = -(0.5 * (g * g));
        }
        __syncthreads();
        if (writer) {
            cout[b] = s;
            const unsigned long long mine = (1ull << 32) | (s.active ? 1ull : 0ull);
            const unsigned long long seen =
                __hip_atomic_fetch_add(count, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + mine;
            if ((int)(seen >> 32) == nobj) {   // the last object: every count is in `seen`
                __hip_atomic_store(count, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int word = 4 * n + ((seen & 0xffffffffull) != 0 ? 1 : 2);
                dstat[0] = word;
                if (hstat != nullptr) {
                    __threadfence_system();
                    reinterpret_cast<volatile int*>(hstat)[n & 3] = word;
                }
            }
        }
    } else {
        if (tid == 0) s = cin[b];
        __syncthreads();
    }
    if (!s.active) return;
    // the ns time rows of this object, the weights read once for all of them (time_row's sums per row)
    if (tid < 64) {   // x_proj = x[:, None] * W[None, :] * 2 * np.pi (scorenet.py:87)
        for (int q = 0; q < ns; ++q) {
            const float av = fmul(fmul(fmul(s.t32[q], w.gfp_w[tid]), 2.0f), 3.14159265358979323846f);
            emb[q * 128 + tid] = sinf(av);
            emb[q * 128 + 64 + tid] = cosf(av);
        }
    }
    for (int i = ns * 128 + tid; i < 6 * 128; i += HT) emb[i] = 0.f;   // unused rows: defined
    __syncthreads();
    if (tid < 128) {
        float d[6];
        dot_chains_multi<128, 16, 6>(w.te_w_t + tid, 128, emb, 128, d);
#pragma unroll
        for (int q = 0; q < 6; ++q) tf[q * 128 + tid] = fmaxf(d[q] + w.te_b[tid], 0.f);
    }
    __syncthreads();
    constexpr int PER = 768 / ODE_OBJ_CHUNKS;
    for (int o = blockIdx.y * PER + tid; o < blockIdx.y * PER + PER; o += HT) {
        float d[6];
        dot_chains_multi<128, 16, 6>(w.h1t_t + o, 768, tf, 128, d);
        const float po = pobj[(size_t)b * 768 + o];
#pragma unroll
        for (int q = 0; q < 6; ++q)
            if (q < ns) init[((size_t)q * nobj + b) * 768 + o] = fadd(po, d[q]);   // the trunks' pov + tpv
    }
}

// res.y[:, -1] of every object: with t_eval set and the solve finished, the dense output of the object's last
// accepted step at te (ode_dense_kernel's expressions with the object's t_old and h = t - t_old; its K_0..K_6 and
// y, the step's start, are in place); else its state (y_new while the accepted step is not copied, else y).
struct OdeObjFinalArgs {
    const OdeObjRec* rec;
    const double* y;
    const double* ynew;
    const double* k[ODE_NK];
    double P[ODE_NK][4];
    double te;
    int dense, kper;
    long long n;
    double* out;
};
__global__ __launch_bounds__(256) void ode_obj_final_kernel(OdeObjFinalArgs a) {
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.n) return;
    const OdeObjRec* rc = a.rec + (e / 9) / a.kper;
    if (!(a.dense && rc->status > 0)) {
        a.out[e] = rc->pend ? a.ynew[e] : a.y[e];
        return;
    }
    double Q[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        double acc = a.k[0][e] * a.P[0][m];
        for (int j = 1; j < ODE_NK; ++j) acc = acc + a.k[j][e] * a.P[j][m];
        Q[m] = acc;
    }
    const double h = rc->t - rc->t_old;
    const double x = (a.te - rc->t_old) / h;
    const double p1 = x, p2 = p1 * x, p3 = p2 * x, p4 = p3 * x;
    const double d = ((Q[0] * p1 + Q[1] * p2) + Q[2] * p3) + Q[3] * p4;
    a.out[e] = h * d + a.y[e];
}

__global__ void ode_obj_fill_kernel(float* __restrict__ p, int n, float v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

int ode_obj_launch_control(const gp_head_weights* w, const float* pobj, const OdeObjRec* cin, OdeObjRec* cout,
                           const double* rowsq, int decide, int prepare, int ns, const OdeConsts& kc, int kper, int nobj,
                           float* init, unsigned long long* count, int* hstat, int* dstat, int n, hipStream_t stream) {
    hipLaunchKernelGGL(ode_obj_control_kernel, dim3(nobj, ODE_OBJ_CHUNKS), dim3(HT), 0, stream, *w, pobj, cin, cout,
                       rowsq, decide, prepare, ns, kc, kper, nobj, init, count, hstat, dstat, n);
    return gp_check_launch("ode_obj_control_kernel");
}

int ode_obj_launch_fill(float* p, int n, float v, hipStream_t stream) {
    hipLaunchKernelGGL(ode_obj_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, p, n, v);
    return gp_check_launch("ode_obj_fill_kernel");
}

int ode_obj_solve(const OdeObjSolve& s, const std::function<int(const OdeObjRec*, int)>& stages,
                  const std::function<int(bool)>& init_norms, const OdeObjRec** fin, int* status_out, int* nfev_out,
                  bool* failed) {
    const int nobj = s.nobj;
    const hipStream_t stream = s.stream;
    OdeObjRec* const rec = s.rec;
    StatusLease status;
    GP_REQUIRE(status.acquire(stream) == 0, "%s: pinned status word / event", s.who);
    const double t0 = s.t0, tf = s.t_bound, dir = tf > t0 ? 1.0 : -1.0;
    const double dscale = diff_scale();
    // every norm of an object runs over its k rows' entries
    const OdeConsts kc = {tf, dir, s.rtol, s.atol, kSigMin, kBase, dscale, (double)s.k * (double)s.entries, 0};
    int rc;
    GP_REQUIRE(hipMemsetAsync(s.count, 0, 256, stream) == hipSuccess, "%s: counter", s.who);
    if ((rc = ode_obj_launch_fill(s.zrow, 768, -0.0f, stream))) return rc;

    // ---- select_initial_step (scipy common.py) per object, with ode_sample_impl's scalar functions
    std::vector<OdeObjRec> hrec((size_t)nobj);
    std::vector<double> hn((size_t)nobj * 3), h0v((size_t)nobj);
    // one evaluation on host-built records: upload, their rows of slot 0, the stage, the norms and their read-back
    auto probe = [&](int parity, int single) -> int {
        OdeObjRec* r = rec + (size_t)parity * nobj;
        GP_TRY(ode_copy_sync(r, hrec.data(), sizeof(OdeObjRec) * (size_t)nobj, hipMemcpyHostToDevice, stream, s.who,
                             "records"));
        int prc;
        if ((prc = ode_obj_launch_control(s.w, s.pobj, r, nullptr, nullptr, 0, 0, 1, kc, s.k, nobj, s.init, s.count,
                                          nullptr, s.dstat, 0, stream)) ||
            (prc = stages(r, single)) || (prc = init_norms(single == 2)))
            return prc;
        return ode_copy_sync(hn.data(), s.norms, sizeof(double) * 3 * (size_t)nobj, hipMemcpyDeviceToHost, stream, s.who,
                             "norm read");
    };
    {   // f(t0)
        OdeObjRec r = {};
        r.t = t0;
        r.active = 1;
        r.t32[0] = (float)t0;
        r.sig[0] = sigma32(r.t32[0]);
        r.coef[0] = ode_coef_t0(r.t32[0], dscale);
        for (int b = 0; b < nobj; ++b) hrec[(size_t)b] = r;
    }
    if ((rc = probe(0, 1))) return rc;
    const double interval = fabs(tf - t0);
    for (int b = 0; b < nobj; ++b) {   // f(t0 + h0 dir, y0 + h0 dir f0)
        const double h0 = ode_init_h0(hn[3 * (size_t)b], hn[3 * (size_t)b + 1], interval);
        h0v[(size_t)b] = h0;
        const double t = t0 + h0 * dir;
        OdeObjRec& r = hrec[(size_t)b];
        r.h = h0 * dir;
        r.t32[0] = (float)t;
        r.sig[0] = sigma32((float)t);
        r.coef[0] = ode_coef(t, dscale);
    }
    if ((rc = probe(1, 2))) return rc;
    for (int b = 0; b < nobj; ++b) {
        OdeObjRec r = {};
        r.t = t0;
        r.h_abs = ode_init_h_abs(h0v[(size_t)b], hn[3 * (size_t)b + 1], hn[3 * (size_t)b + 2], interval);
        r.nfev = 2;
        hrec[(size_t)b] = r;
    }
    GP_TRY(ode_copy_sync(rec, hrec.data(), sizeof(OdeObjRec) * (size_t)nobj, hipMemcpyHostToDevice, stream, s.who,
                         "records"));

    // ---- the attempts, one enqueued ahead of the status read; the loop ends when no object runs
    int* hs_dev = status.map(true);
    auto launch = [&](int at, int what) -> int {
        OdeObjRec* prepared = rec + (size_t)((at + 1) & 1) * nobj;
        int lrc = GP_OK;
        if (what & 1)   // decides attempt at - 1, prepares attempt at
            lrc = ode_obj_launch_control(s.w, s.pobj, rec + (size_t)(at & 1) * nobj, prepared, s.rowsq, at > 0 ? 1 : 0, 1,
                                         6, kc, s.k, nobj, s.init, s.count, hs_dev, s.dstat, at, stream);
        return (lrc || !(what & 2)) ? lrc : stages(prepared, 0);
    };
    int at = 0;
    if ((rc = ode_run_attempts(status, hs_dev, true, launch, [&](int) { return s.dstat; }, s.who, &at))) return rc;
    *fin = rec + (size_t)((at + 2) & 1) * nobj;
    GP_TRY(ode_copy_sync(hrec.data(), *fin, sizeof(OdeObjRec) * (size_t)nobj, hipMemcpyDeviceToHost, stream, s.who,
                         "final records"));
    status.pending = false;
    bool bad = false;
    for (int b = 0; b < nobj; ++b) {
        if (status_out) status_out[b] = hrec[(size_t)b].status;
        if (nfev_out) nfev_out[b] = hrec[(size_t)b].nfev;
        bad = bad || hrec[(size_t)b].status < 0;
    }
    if (failed) *failed = bad;
    return GP_OK;
}

namespace {
struct OdeObjLayout {
    OdeStateBlock st;
    size_t xout, den_ws, total;
    OdeObjTail tail;
};
OdeObjLayout ode_obj_layout(int rows, int nobj) {
    OdeObjLayout L = {};
    size_t off = 0;
    L.st = ode_state_layout(off, rows, 9);
    L.xout = off; off += align256((size_t)rows * 9 * sizeof(double));
    L.tail = ode_obj_tail_layout(off, rows, nobj);
    L.den_ws = off; off += align256(gp_ode_workspace_size(rows));
    L.total = off;
    return L;
}
}  // namespace

extern "C" size_t gp_ode_object_workspace_size_k(int rows, int k) {
    return (rows >= 1 && k >= 1 && rows % k == 0) ? ode_obj_layout(rows, rows / k).total : 0;
}
// enough for every k (k = 1: one record and six rows per candidate)
extern "C" size_t gp_ode_object_workspace_size(int rows) { return gp_ode_object_workspace_size_k(rows, 1); }

extern "C" int gp_ode_sample_object(const gp_head_weights* w, const float* pobj, const float* x0, int rows, int k,
                                    int rows_total, double T0, double eps, int steps, double rtol, double atol,
                                    const float* pts_center, double* pose, double* q, int* nfev_out, int* status_out,
                                    void* workspace, size_t workspace_bytes, hipStream_t stream) {
    GP_REQUIRE(w && pobj && x0 && pts_center && pose && q && workspace && rows >= 1 && k >= 1 && steps >= 0,
               "ode_sample_object: bad arguments");
    GP_REQUIRE(rows % k == 0, "ode_sample_object: rows %d are not whole objects of k = %d", rows, k);
    GP_REQUIRE(rows_total >= rows && rows_total % k == 0,
               "ode_sample_object: rows_total %d must be whole objects and hold this call's %d rows", rows_total, rows);
    GP_REQUIRE(T0 != eps, "ode_sample_object: empty integration interval (T0 == eps)");
    GP_REQUIRE(steps != 1, "ode_sample_object: steps must be 0 (t_eval unset) or >= 2");
    const int nobj = rows / k;
    const OdeObjLayout L = ode_obj_layout(rows, nobj);
    GP_REQUIRE(workspace_bytes >= L.total,
               "ode_sample_object: workspace too small (gp_ode_object_workspace_size_k(rows, k))");
    char* ws = static_cast<char*>(workspace);
    auto dptr = [&](size_t off) { return reinterpret_cast<double*>(ws + off); };
    const OdeObjSolve sv(w, pobj, nobj, k, 9, T0, eps, rtol, atol, ws, L.tail, stream, "ode_sample_object");
    const long long n = (long long)rows * 9;
    const int nt = ode_nt(w, rows_total);   // the whole batch's tile class
    const int nwg = (rows + 16 * nt - 1) / (16 * nt);

    double* K[ODE_NK];
    for (int j = 0; j < ODE_NK; ++j) K[j] = dptr(L.st.k[j]);
    OdeObjArgs a = ode_obj_args<OdeObjArgs>(w, sv.init, sv.zrow, dptr(L.st.y), dptr(L.st.ynew), K, dptr(L.st.f1),
                                            sv.rowsq, rtol, atol, rows, k);
    const OdeTableau tb = ode_tableau();
    auto stages = [&](const OdeObjRec* r, int single) {
        a.rec = r;
        a.single = single;
        const dim3 grid(nwg), blk(EVAL_WV * 64);
        head_dispatch(w->pe2_h ? X3P : 0, nt, [&](auto pl, auto ntc) {
            hipLaunchKernelGGL((ode_obj_attempt_kernel<pl.value, ntc.value>), grid, blk, 0, stream, a, tb);
        });
        return gp_check_launch("ode_obj_attempt_kernel");
    };
    auto init_norms = [&](bool with_f1) {
        hipLaunchKernelGGL(ode_obj_init_norms_kernel<9>, dim3(nobj), dim3(64), 0, stream, (const double*)a.y,
                           (const double*)a.k[0], (const double*)(with_f1 ? a.f1 : nullptr), rows, k, atol, rtol,
                           sv.norms);
        return gp_check_launch("ode_obj_init_norms_kernel");
    };
    int rc;
    hipLaunchKernelGGL(f32_to_f64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x0, a.y, n);
    if ((rc = gp_check_launch("f32_to_f64_kernel"))) return rc;
    const OdeObjRec* fin = nullptr;
    bool failed = false;
    if ((rc = ode_obj_solve(sv, stages, init_norms, &fin, status_out, nfev_out, &failed))) return rc;
    GP_REQUIRE(!(failed && steps > 0),
               "ode_sample_object: RK45 failed (step size below the spacing of t) with t_eval set: the collected "
               "t_eval outputs need the host controller (genpose2_amd/ode.py rk45_drive)");
    OdeObjFinalArgs fa = {};
    fa.rec = fin;
    fa.y = a.y;
    fa.ynew = a.ynew;
    for (int j = 0; j < ODE_NK; ++j) {
        fa.k[j] = a.k[j];
        for (int m = 0; m < 4; ++m) fa.P[j][m] = kP74[j * 4 + m];
    }
    fa.te = eps;
    fa.dense = steps > 0;
    fa.kper = k;
    fa.n = n;
    fa.out = dptr(L.xout);
    hipLaunchKernelGGL(ode_obj_final_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, fa);
    if ((rc = gp_check_launch("ode_obj_final_kernel"))) return rc;
    // ---- denoise (samplers.py:240-249) with eps's scalars
    return ode_denoise_impl(w, pobj, ode_denoise_scalars(eps, steps), fa.out, rows, k, rows_total, pts_center, pose, q,
                            ws + L.den_ws, gp_ode_workspace_size(rows), stream);
}

// Test aid: one launch of ode_obj_control_kernel as gp_ode_sample_object launches it for an attempt (prepare = 1,
// six time rows, the sampler's sigma constants), on caller-owned device buffers. rec_in / rec_out: nobj records of
// gp_debug_ode_obj_rec_size() bytes each; rowsq (nobj * kper) the rows' error sums, read when decide != 0;
// init (6, nobj, 768); count: one zeroed 64-bit word; host_status: NULL or 4 host-mapped ints as the device
// addresses them; dev_status: one int. Not part of the sampler's ABI contract.
extern "C" size_t gp_debug_ode_obj_rec_size(void) { return sizeof(OdeObjRec); }

extern "C" int gp_debug_ode_obj_control(const gp_head_weights* w, const float* pobj, const void* rec_in, void* rec_out,
                                        const double* rowsq, int decide, int n, double t_bound, double direction,
                                        int kper, int nobj, float* init, unsigned long long* count, int* host_status,
                                        int* dev_status, hipStream_t stream) {
    GP_REQUIRE(w && pobj && rec_in && rec_out && init && count && dev_status && kper >= 1 && nobj >= 1 && n >= 0,
               "debug_ode_obj_control: bad arguments");
    GP_REQUIRE(!decide || rowsq, "debug_ode_obj_control: decide without row sums");
    const OdeConsts kc = {t_bound, direction, 0.0, 0.0, kSigMin, kBase, diff_scale(), (double)kper * 9.0, 0};
    hipLaunchKernelGGL(ode_obj_control_kernel, dim3(nobj, ODE_OBJ_CHUNKS), dim3(HT), 0, stream, *w, pobj,
                       static_cast<const OdeObjRec*>(rec_in), static_cast<OdeObjRec*>(rec_out), rowsq,
                       decide ? 1 : 0, 1, 6, kc, kper, nobj, init, count, host_status, dev_status, n);
    return gp_check_launch("ode_obj_control_kernel<debug>");
}
