// What the ODE sampler's translation units share: the controller record, the stage arguments, the stage
// arithmetic (one definition each) and the host-side launch helpers of gp_ode.hip that gp_ode_energy.hip calls.
// The score agent's stage kernels live in gp_ode.hip, the energy agent's (the same stages around the gradient
// trunk and its reverse pass) in gp_ode_energy.hip: a translation unit of their own, so that they cannot move the
// register assignment of the kernels that were there before them.
#pragma once
#include "gp_head.h"

#define ODE_NK 7   // Dormand-Prince stages incl. the FSAL derivative

// Device-resident RK45 controller state (the device-controlled path, gp_ode_auto_*). One copy per
// attempt parity: the control kernel of attempt n reads ctl[n & 1] and writes ctl[(n + 1) & 1], the
// stage kernels of attempt n read ctl[(n + 1) & 1]. Field order fixed (doubles, floats, ints) so the
// host mirror (genpose2_amd/ode.py OdeCtl) has the same layout.
struct OdeCtl {
    double t, h_abs;              // solver time; step size carried to the next step (scipy self.h_abs)
    double t_old, h_last;         // last accepted step (dense output)
    double h, t_new, h_abs_loc;   // the prepared attempt (scipy _step_impl locals h, t_new, h_abs)
    double coef[6];               // -(0.5 g(t_s)^2) of the attempt's 6 stage times
    float t32[6], sig[6];         // float32(t_s), sigma(t32)
    int status;                   // 0 running, 1 finished, -1 step size below spacing (scipy failure)
    int active;                   // the prepared attempt runs
    int rejected;                 // scipy step_rejected within the current step
    int nfev, n_acc, yi;          // RHS evaluations, accepted steps, y buffer holding the state
    int kidx[ODE_NK];             // K slot permutation (FSAL swaps slots 0 and 6 on acceptance)
};
static_assert(sizeof(OdeCtl) == 208, "OdeCtl layout is mirrored on the host");

struct OdeStageArgs {
    gp_head_weights w;
    const float* pobj;
    const float* tproj;          // (768) time row of this stage's t (host-controlled calls)
    float sigma;                 // sigma(t32), fp32 (score = f / (sigma + 1e-7))
    double coef;                 // -(0.5 * g(t)^2)
    const double* y;             // (R,9) state at the step's start
    const double* k[ODE_NK];     // stage derivatives combined into this stage's input
    double a[ODE_NK];            // y_in = y + (sum_{j<nk} a_j K_j) * h
    int nk;
    double h;
    double* kout;                // (R,9) this stage's derivative
    // final stage of an attempt (MODE 1): y_new out and the error-estimator partials
    double* ynew;
    double e[ODE_NK];            // error weights over K_0..K_6 (K_6 = this stage)
    double rtol, atol;
    double* part;                // (nwg) sum over the workgroup's elements of (err/scale)^2
    int part_off;                // index of this launch's first partial (global-batch shards: the single call's
                                 // workgroup index of this shard's first row tile; 0 otherwise)
    int rows, kper;
    // device-controlled attempts: state, time rows and buffers resolved from ctl
    const OdeCtl* ctl;           // null for host-controlled calls
    const float* tproj6;         // (6,768) rows of the prepared attempt
    double* ybuf[2];
    double* kbuf[ODE_NK];
    int stage;                   // 1..6
};

// The stage arithmetic the sampler's and the likelihood's stage kernels share, one definition each: a last-bit
// difference in any of them can flip an accept / reject of the step controller.
// y_in = y + (sum_{j<nk} a_j K_j) h of entry e, nk >= 1 (scipy rk.py rk_step's order)
__device__ __forceinline__ double ode_stage_in(const double* const* kin, const double* acoef, int nk, double h, size_t e,
                                               double yv) {
#pragma clang fp contract(off)
    double acc = kin[0][e] * acoef[0];
    for (int s = 1; s < nk; ++s) acc = acc + kin[s][e] * acoef[s];
    return yv + acc * h;
}
// scipy's error term of entry e: err = (K^T E) h / scale, scale = atol + max(|y|, |y_new|) rtol; kv = K_6[e], the
// derivative this stage just formed
template <typename Args>   // OdeStageArgs, or the per-object OdeObjArgs (e, atol, rtol)
__device__ __forceinline__ double ode_err_term(const Args& a, const double* const* kin, double kv, double h,
                                               size_t e, double y0, double y1) {
#pragma clang fp contract(off)
    double acc = kin[0][e] * a.e[0];
    for (int s = 1; s < ODE_NK - 1; ++s) acc = acc + kin[s][e] * a.e[s];
    acc = acc + kv * a.e[ODE_NK - 1];
    const double sc = a.atol + fmax(fabs(y0), fabs(y1)) * a.rtol;
    return (acc * h) / sc;
}
// The workgroup's sum of the threads' sq in a fixed order (xor tree per wave, waves in order) -> *out; esq: one
// double of LDS per wave
__device__ __forceinline__ void ode_block_partial(double sq, double* esq, double* out) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sq += __shfl_xor(sq, off, 64);
    if ((tid & 63) == 0) esq[tid >> 6] = sq;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int v = 0; v < EVAL_WV; ++v) t += esq[v];
        *out = t;
    }
}

// The tableau of a fused attempt (ode_attempt_kernel), passed by value
struct OdeTableau {
    double A[36], B[6];
};

// Final denoise (samplers.py:240-249) + epilogue: the arguments of ode_denoise_kernel
struct OdeDenoiseArgs {
    gp_head_weights w;
    const float* pobj;
    const float* tproj;
    float sigma;
    float g2;        // diffusion(eps)^2 in fp32
    float step;      // (1 - eps) / num_steps as fp32
    const double* x;
    const float* center;
    double* pose;
    double* q;
    int rows, kper;
};

// ------------------------------------------------------------------------------ host side, gp_ode.hip
// Time rows of nt <= 6 stage times into the first nt x 768 floats of ws (ode_time_rows_kernel)
int ode_launch_times(const gp_head_weights* w, const float* t32, int nt, void* ws, hipStream_t stream);
// out[0] = sqrt(sum(part[0..n))) / sqrt(count) (ode_norm_kernel)
int ode_launch_norm(const double* part, int n, double count, double* out, hipStream_t stream);
// Byte offset of the error partials in a host-controlled workspace (behind the 6 time rows)
size_t ode_part_offset();

// ------------------------------------------------------------------------------ host side, gp_ode_energy.hip
// The energy agent's stages: 16-row tiles, exact fp32. Each returns gp_check_launch's status.
bool ode_energy_weights_ok(const gp_head_grad_weights* gw);
int ode_energy_launch_stage(const OdeStageArgs& a, const gp_head_grad_weights& gw, bool last, hipStream_t stream);
int ode_energy_launch_attempt(const OdeStageArgs& a, const gp_head_grad_weights& gw, const OdeTableau& tb,
                              hipStream_t stream);
