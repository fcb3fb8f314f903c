// The probability-flow ODE sampler's stages for the energy agent (agent_type='energy').
//
// Reference: cond_ode_sampler (networks/gf_algorithms/samplers.py:204-219) calls score_model(data) whichever agent
// it samples, and PoseEnergyNet.forward(return_item='score') (energynet.py:211-233) answers with grad_x E,
// E = sum_o x_o f_o(x) / sigma. Here a stage is gp_ode.hip's stage with that score in place of f / (sigma + 1e-7):
// the gradient form of the exact-fp32 trunk and its reverse pass (gp_head.h head_trunk<.., GRAD>, head_backward on
// the transposed weights), s = f / sigma + J_f^T (x / sigma) as head_grad_eval_kernel (gp_score.hip) forms it --
// plain sigma, the head output behind an opaque copy in front of pose_grad's sum -- so a stage's score equals
// gp_energy_score_eval on float(y_in) bit for bit. The prologue (ode_stage_in), K = coef * (double)s, y_new, the
// error terms (ode_err_term) and the workgroup partial (ode_block_partial) are gp_ode.h's, one definition each.
// Tiles are 16 rows and 8 waves, exact fp32 whatever arithmetic the score kernels run (the reverse pass has no
// f16x3 form). The control, norm, dense-output, time-row and init-norm kernels are gp_ode.hip's, unchanged, and
// the entries at the end of this file are gp_ode.h's host sequences (ode_rhs_once, ode_attempt_host,
// ode_denoise_begin) around this file's launches.
//
// A translation unit of its own: a sibling instantiation in gp_score.hip once moved the register assignment of
// pc_step_kernel<1,8,0> (DESIGN "Energy model as a score model"); gp_ode.hip's kernels compile to the assembly
// they had before this file existed.
#include "gp_ode.h"

namespace {

// One RK45 stage for the workgroup's 16 rows (ode_stage_body's energy form). MODE 0: stage derivative. MODE 1:
// last stage of an attempt (y_new, K_6, error partials). y_in = y + (sum_{j<nk} acoef_j K_j) h,
// K_out = coef * grad_x E(f32(y_in), t).
template <int MODE>
__device__ __forceinline__ void ode_energy_stage_body(const OdeStageArgs& a, const gp_head_grad_weights& gw,
                                                      const double* y, const double* const* kin, const double* acoef,
                                                      int nk, double h, double coef, float sigma, const float* tproj,
                                                      double* kout, double* ynew, HeadSmem<1, EVAL_WV, 0>& sm,
                                                      GradSmem& gs, int* obj, double* y0s, double* y1s, double* esq) {
    constexpr int NTH = EVAL_WV * 64;
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * 16;
    stage_small_weights(a.w, sm);
    for (int i = tid; i < 16 * 16; i += NTH) {
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
    if (tid < 16) obj[tid] = obj_of_row(r0 + tid, a.rows, a.kper);
    head_trunk<1, EVAL_WV, false, true>(a.w, a.pobj, tproj, obj, sm, 0, &gs, sigma);
    head_backward<EVAL_WV>(gw, sm, gs);
    double sq = 0.0;   // this thread's (err/scale)^2 term: a lane per (row, output)
    if (tid < 16 * 9) {
#pragma clang fp contract(off)
        const int c = tid / 9, o = tid - c * 9;
        const int r = r0 + c;
        float f = fdiv(head_out(sm, c, o), sigma);
        asm volatile("" : "+v"(f));   // keeps head_out's sum apart from pose_grad's (head_grad_eval_kernel)
        const float s = fadd(f, pose_grad<EVAL_WV>(gs, c, o));
        if (r < a.rows) {
            const size_t e = (size_t)r * 9 + o;
            const double kv = coef * (double)s;
            kout[e] = kv;
            if (MODE == 1) {
                const double er = ode_err_term(a, kin, kv, h, e, y0s[tid], y1s[tid]);
                sq = er * er;
            }
        }
    }
    if (MODE == 1) ode_block_partial(sq, esq, &a.part[a.part_off + blockIdx.x]);
}

// ode_stage_kernel's energy form (host-controlled calls, and the device-controlled attempts launched stage by
// stage under GENPOSE2_ODE_FUSED=0)
template <int MODE>
__global__ __launch_bounds__(EVAL_WV * 64) void ode_energy_stage_kernel(OdeStageArgs a, gp_head_grad_weights gw) {
    __shared__ HeadSmem<1, EVAL_WV, 0> sm;
    __shared__ GradSmem gs;
    __shared__ int obj[16];
    __shared__ double y0s[16 * 9], y1s[16 * 9], esq[EVAL_WV];
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
    ode_energy_stage_body<MODE>(a, gw, y, kin, a.a, a.nk, h, coef, sigma, tproj, kout, ynew, sm, gs, obj, y0s, y1s,
                                esq);
}

// ode_attempt_kernel's energy form: the six stages of a device-controlled attempt in one launch. The barrier
// between two stages retires the earlier stage's K stores, its reads of the staged weights and the epilogue's
// reads of the head outputs and the reverse pass's partial tiles, which the next stage rewrites.
__global__ __launch_bounds__(EVAL_WV * 64) void ode_energy_attempt_kernel(OdeStageArgs a, gp_head_grad_weights gw,
                                                                          OdeTableau tb) {
    __shared__ HeadSmem<1, EVAL_WV, 0> sm;
    __shared__ GradSmem gs;
    __shared__ int obj[16];
    __shared__ double y0s[16 * 9], y1s[16 * 9], esq[EVAL_WV];
    __shared__ double tab[42];
    __shared__ const double* kin[ODE_NK];
    const OdeCtl* c = a.ctl;
    if (!c->active) return;
    ode_attempt_to_lds(a, c, tb, tab, kin);
    const double* y = a.ybuf[c->yi];
    const double h = c->h;
    __syncthreads();
    for (int s = 1; s < 6; ++s) {
        if (s > 1) __syncthreads();
        ode_energy_stage_body<0>(a, gw, y, kin, tab + s * 6, s, h, c->coef[s - 1], c->sig[s - 1],
                                 a.tproj6 + (size_t)(s - 1) * 768, const_cast<double*>(kin[s]), nullptr, sm, gs, obj,
                                 y0s, y1s, esq);
    }
    __syncthreads();
    ode_energy_stage_body<1>(a, gw, y, kin, tab + 36, 6, h, c->coef[5], c->sig[5], a.tproj6 + (size_t)5 * 768,
                             const_cast<double*>(kin[6]), a.ybuf[c->yi ^ 1], sm, gs, obj, y0s, y1s, esq);
}

// ode_denoise_kernel's energy form: grad = grad_x E(float(x), eps) in fp32, then the same update and epilogue.
__global__ __launch_bounds__(EVAL_WV * 64) void ode_energy_denoise_kernel(OdeDenoiseArgs a, gp_head_grad_weights gw) {
    __shared__ HeadSmem<1, EVAL_WV, 0> sm;
    __shared__ GradSmem gs;
    __shared__ int obj[16];
    __shared__ double xm[16 * 9];
    constexpr int NTH = EVAL_WV * 64;
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * 16;
    stage_small_weights(a.w, sm);
    for (int i = tid; i < 16 * 16; i += NTH) {
        const int c = i >> 4, j = i & 15;
        const int r = r0 + c;
        sm.xin[i] = (r < a.rows && j < 9) ? (float)a.x[(size_t)r * 9 + j] : 0.f;
    }
    if (tid < 16) obj[tid] = obj_of_row(r0 + tid, a.rows, a.kper);
    head_trunk<1, EVAL_WV, false, true>(a.w, a.pobj, a.tproj, obj, sm, 0, &gs, a.sigma);
    head_backward<EVAL_WV>(gw, sm, gs);
    if (tid < 16 * 9) {
#pragma clang fp contract(off)
        const int c = tid / 9, o = tid - c * 9;
        const int r = r0 + c;
        float f = fdiv(head_out(sm, c, o), a.sigma);
        asm volatile("" : "+v"(f));
        const float grad = fadd(f, pose_grad<EVAL_WV>(gs, c, o));
        if (r < a.rows) {
            const float drift = 0.0f - a.g2 * grad;
            xm[tid] = a.x[(size_t)r * 9 + o] + (double)(drift * a.step);
        }
    }
    __syncthreads();
    if (tid < 16 && r0 + tid < a.rows) {
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

}  // namespace

// ------------------------------------------------------------------------------ launches (gp_ode.h)
bool ode_energy_weights_ok(const gp_head_grad_weights* gw) { return gw && gw->pe0_wt && gw->pe2_wt && gw->h1p_wt; }

int ode_energy_launch_stage(const OdeStageArgs& a, const gp_head_grad_weights& gw, bool last, hipStream_t stream) {
    const dim3 grid((a.rows + 15) / 16), blk(EVAL_WV * 64);
    if (last)
        hipLaunchKernelGGL(ode_energy_stage_kernel<1>, grid, blk, 0, stream, a, gw);
    else
        hipLaunchKernelGGL(ode_energy_stage_kernel<0>, grid, blk, 0, stream, a, gw);
    return gp_check_launch("ode_energy_stage_kernel");
}

int ode_energy_launch_attempt(const OdeStageArgs& a, const gp_head_grad_weights& gw, const OdeTableau& tb,
                              hipStream_t stream) {
    hipLaunchKernelGGL(ode_energy_attempt_kernel, dim3((a.rows + 15) / 16), dim3(EVAL_WV * 64), 0, stream, a, gw, tb);
    return gp_check_launch("ode_energy_attempt_kernel");
}

// ------------------------------------------------------------------------------ C ABI
// The workspaces are the score entries': 6 time rows | one error partial per 16 rows, which is this tiling's count.
extern "C" int gp_ode_rhs_energy(const gp_head_weights* w, const gp_head_grad_weights* gw, const float* pobj,
                                 float t32, float sigma, double coef, const double* y, const double* const* kin,
                                 const double* acoef, int nk, double h, int rows, int k, double* kout,
                                 void* workspace, size_t workspace_bytes, hipStream_t stream) {
    GP_REQUIRE(ode_energy_weights_ok(gw) && sigma > 0.f, "ode_rhs_energy: bad arguments");
    return ode_rhs_once("ode_rhs_energy", w, pobj, t32, sigma, coef, y, kin, acoef, nk, h, rows, k, kout, workspace,
                        workspace_bytes, stream,
                        [&](const OdeStageArgs& a) { return ode_energy_launch_stage(a, *gw, false, stream); });
}

extern "C" int gp_ode_attempt_energy(const gp_head_weights* w, const gp_head_grad_weights* gw, const float* pobj,
                                     const float* t32_6, const float* sigma_6, const double* coef_6, const double* y,
                                     double* const* kslots, const double* tableau_a, const double* b,
                                     const double* e, double h, double rtol, double atol, int rows, int k,
                                     double* ynew, double* err_out, void* workspace, size_t workspace_bytes,
                                     hipStream_t stream) {
    GP_REQUIRE(ode_energy_weights_ok(gw) && sigma_6, "ode_attempt_energy: bad arguments");
    for (int s = 0; s < 6; ++s) GP_REQUIRE(sigma_6[s] > 0.f, "ode_attempt_energy: sigma must be positive");
    return ode_attempt_host(
        "ode_attempt_energy", w, pobj, t32_6, sigma_6, coef_6, y, kslots, tableau_a, b, e, h, rtol, atol, rows, k, ynew,
        err_out, workspace, workspace_bytes, stream, [&] { return (rows + 15) / 16; }, (double)rows * 9.0,
        [&](const OdeStageArgs& a, bool last) { return ode_energy_launch_stage(a, *gw, last, stream); });
}

extern "C" int gp_ode_denoise_energy(const gp_head_weights* w, const gp_head_grad_weights* gw, const float* pobj,
                                     float t32, float sigma, float g2, float step, const double* x, int rows, int k,
                                     const float* pts_center, double* pose, double* q, void* workspace,
                                     size_t workspace_bytes, hipStream_t stream) {
    GP_REQUIRE(ode_energy_weights_ok(gw) && sigma > 0.f, "ode_denoise_energy: bad arguments");
    OdeDenoiseArgs a;
    GP_TRY(ode_denoise_begin("ode_denoise_energy", w, pobj, t32, sigma, g2, step, x, rows, k, pts_center, pose, q,
                             workspace, workspace_bytes, stream, &a));
    hipLaunchKernelGGL(ode_energy_denoise_kernel, dim3((rows + 15) / 16), dim3(EVAL_WV * 64), 0, stream, a, *gw);
    return gp_check_launch("ode_energy_denoise_kernel");
}
