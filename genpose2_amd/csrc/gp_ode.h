// What the ODE sampler's translation units share: the controller record, the stage arguments, the stage
// arithmetic (one definition each) and the host-side launch helpers of gp_ode.hip that gp_ode_energy.hip calls.
// The score agent's stage kernels live in gp_ode.hip, the energy agent's (the same stages around the gradient
// trunk and its reverse pass) in gp_ode_energy.hip: a translation unit of their own, so that they cannot move the
// register assignment of the kernels that were there before them. The per-object likelihood (gp_like_object.hip, its
// own translation unit for the same reason) takes the per-object controller's record, constants and launch, the
// tableau and the status reads of the whole-sampler entries from here.
#pragma once
#include <cmath>
#include <mutex>
#include <vector>

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

// Constants of a device step controller (ode_control_kernel, ode_obj_control_kernel)
struct OdeConsts {
    double t_bound, direction, rtol, atol;
    double sig_min, base, diff_scale;   // sigma(t) = sig_min * base^t; g = sigma(t) * diff_scale
    double count;                       // elements of the state (R*9) for the RMS norm
    int nwg;                            // error partials
};

// The per-object controller record (gp_ode_sample_object, gp_like_sample_object; see gp_ode.hip)
struct OdeObjRec {
    double t, h_abs;              // solver time; step size carried to the next step (scipy self.h_abs)
    double t_old;                 // start of the last accepted step (dense output; its h is t - t_old)
    double h, t_new, h_abs_loc;   // the prepared attempt (scipy _step_impl locals h, t_new, h_abs)
    double coef[6];               // -(0.5 g(t_s)^2) of the attempt's 6 stage times
    float t32[6], sig[6];         // float32(t_s), sigma(t32)
    int status;                   // 0 running, 1 finished, -1 step size below spacing (scipy failure)
    int active;                   // the prepared attempt runs
    int rejected;                 // scipy step_rejected within the current step
    int nfev, n_acc;              // RHS evaluations, accepted steps
    int pend;                     // the last decided attempt was accepted and y_new / K_6 are not yet copied to
                                  // y / K_0: the state is in y_new
};
static_assert(sizeof(OdeObjRec) == 168, "OdeObjRec: doubles, floats, ints without padding");

// sum_{j<n} v(j) by one wave in an order that is a function of j and n alone: lane l adds j = l, l + 64, ... in
// increasing j from 0, the 64 lane sums meet in an xor tree. Every lane returns the sum.
template <typename F>
__device__ __forceinline__ double ode_obj_wave_sum(int n, F v) {
#pragma clang fp contract(off)
    double t = 0.0;
    for (int j = threadIdx.x & 63; j < n; j += 64) t += v(j);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off, 64);
    return t;
}

// ------------------------------------------------------------------------------ host constants and status reads
// (gp_ode.hip's whole-sampler entries and gp_like_object.hip's)
// Dormand-Prince tableau exactly as scipy's RK45 class attributes (rk.py)
static const double kA6[36] = {0, 0, 0, 0, 0, 0,
                        1.0 / 5, 0, 0, 0, 0, 0,
                        3.0 / 40, 9.0 / 40, 0, 0, 0, 0,
                        44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0, 0,
                        19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0, 0,
                        9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656, 0};
static const double kB6[6] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
static const double kE7[7] = {-71.0 / 57600, 0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};
static const double kP74[28] = {1, -8048581381.0 / 2820520608, 8663915743.0 / 2820520608, -12715105075.0 / 11282082432,
                         0, 0, 0, 0,
                         0, 131558114200.0 / 32700410799, -68118460800.0 / 10900136933, 87487479700.0 / 32700410799,
                         0, -1754552775.0 / 470086768, 14199869525.0 / 1410260304, -10690763975.0 / 1880347072,
                         0, 127303824393.0 / 49829197408, -318862633887.0 / 49829197408, 701980252875.0 / 199316789632,
                         0, -282668133.0 / 205662961, 2019193451.0 / 616988883, -1453857185.0 / 822651844,
                         0, 40617522.0 / 29380423, -110615467.0 / 29380423, 69997945.0 / 29380423};
constexpr double kSigMin = 0.01, kBase = 50.0 / 0.01;

static inline double diff_scale() { return sqrt(2.0 * (log(50.0) - log(0.01))); }
// sigma(t32) as sde.py forms it for a float32 tensor: f32(0.01) * 5000^t32 (power correctly rounded)
static inline float sigma32(float t32) { return 0.01f * (float)pow(kBase, (double)t32); }

static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Host resources of gp_ode_sample's status reads (a pinned int and an event on the stream's device),
// leased from a per-device pool for one call and returned after it. A per-thread cache bound them to
// the first device a thread used, which breaks a host that drives several GPUs from one thread (or a
// cgo host, whose goroutines move between OS threads); creating them per call would cost a
// device-synchronising hipHostFree. The pool holds at most as many readers per device as calls ever
// ran on it at once.
struct StatusReader {
    int* pinned;
    hipEvent_t ev;
    int dev;
};
extern std::mutex g_status_mu;                  // defined in gp_ode.hip
extern std::vector<StatusReader> g_status_pool;

struct StatusLease {
    StatusReader r{nullptr, nullptr, -1};
    hipStream_t stream = nullptr;
    bool pending = false;   // a status copy into r.pinned was enqueued and may not have landed yet
    int acquire(hipStream_t s) {
        stream = s;
        int cur = 0, dev = 0;
        if (hipGetDevice(&cur) != hipSuccess) return -1;
        dev = cur;
        if (s != nullptr && hipStreamGetDevice(s, &dev) != hipSuccess) return -1;
        {
            std::lock_guard<std::mutex> lk(g_status_mu);
            for (size_t i = 0; i < g_status_pool.size(); ++i)
                if (g_status_pool[i].dev == dev) {
                    r = g_status_pool[i];
                    g_status_pool.erase(g_status_pool.begin() + (long)i);
                    return 0;
                }
        }
        if (dev != cur && hipSetDevice(dev) != hipSuccess) return -1;
        r.dev = dev;
        bool ok = hipHostMalloc(reinterpret_cast<void**>(&r.pinned), 64, hipHostMallocDefault) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&r.ev, hipEventDisableTiming) == hipSuccess;
        if (!ok) {   // a partial creation frees what it made (nothing of it is pooled)
            if (r.pinned != nullptr) (void)hipHostFree(r.pinned);
            r.pinned = nullptr;
            r.ev = nullptr;
        }
        if (dev != cur) (void)hipSetDevice(cur);
        return ok ? 0 : -1;
    }
    ~StatusLease() {
        if (r.pinned == nullptr || r.ev == nullptr) return;
        // an early return between the status copy and its wait leaves the copy in flight: it must land
        // before another call can lease this pinned word (if the stream cannot be drained, the reader is
        // dropped rather than pooled)
        if (pending && hipStreamSynchronize(stream) != hipSuccess) return;
        std::lock_guard<std::mutex> lk(g_status_mu);
        g_status_pool.push_back(r);
    }
};

// ------------------------------------------------------------------------------ host side, gp_ode.hip
// Time rows of nt <= 6 stage times into the first nt x 768 floats of ws (ode_time_rows_kernel)
int ode_launch_times(const gp_head_weights* w, const float* t32, int nt, void* ws, hipStream_t stream);
// out[0] = sqrt(sum(part[0..n))) / sqrt(count) (ode_norm_kernel)
int ode_launch_norm(const double* part, int n, double count, double* out, hipStream_t stream);
// Byte offset of the error partials in a host-controlled workspace (behind the 6 time rows)
size_t ode_part_offset();
// One launch of ode_obj_control_kernel (the per-object controller: decides attempt n - 1 from the rows' error sums,
// prepares attempt n and its ns folded time rows), as gp_ode_sample_object launches it
int ode_obj_launch_control(const gp_head_weights* w, const float* pobj, const OdeObjRec* cin, OdeObjRec* cout,
                           const double* rowsq, int decide, int prepare, int ns, const OdeConsts& kc, int kper, int nobj,
                           float* init, unsigned long long* count, int* hstat, int* dstat, int n, hipStream_t stream);
// p[0..n) = v (ode_obj_fill_kernel: the row of -0.0f)
int ode_obj_launch_fill(float* p, int n, float v, hipStream_t stream);

// ------------------------------------------------------------------------------ host side, gp_ode_energy.hip
// The energy agent's stages: 16-row tiles, exact fp32. Each returns gp_check_launch's status.
bool ode_energy_weights_ok(const gp_head_grad_weights* gw);
int ode_energy_launch_stage(const OdeStageArgs& a, const gp_head_grad_weights& gw, bool last, hipStream_t stream);
int ode_energy_launch_attempt(const OdeStageArgs& a, const gp_head_grad_weights& gw, const OdeTableau& tb,
                              hipStream_t stream);
