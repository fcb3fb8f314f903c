// What the ODE sampler's translation units share: the controller record, the stage arguments, the stage
// arithmetic (one definition each) and the host-side launch helpers of gp_ode.hip that gp_ode_energy.hip calls.
// The score agent's stage kernels live in gp_ode.hip, the energy agent's (the same stages around the gradient
// trunk and its reverse pass) in gp_ode_energy.hip: a translation unit of their own, so that they cannot move the
// register assignment of the kernels that were there before them. The per-object likelihood (gp_like_object.hip, its
// own translation unit for the same reason) has its own stage, state and final kernels only: the per-object solve
// between "the state is in y" and "the final records are on the host" is one host driver (ode_obj_solve, defined in
// gp_ode.hip) that gp_ode_sample_object and gp_like_sample_object both call with their stage launch, and the
// select_initial_step scalars, the init-norms kernel, the tableau and the status reads are defined once, here.
// So is the host plumbing around a stage launch, which every entry calls with its own stage launcher: one
// right-hand side (ode_rhs_once), the stages 1..6 of an attempt (ode_run_stages; ode_attempt_host around it for the
// host-controlled entries), the final denoise's arguments and scalars (ode_denoise_begin, ode_denoise_scalars), the
// state block of a whole-solve workspace (ode_state_layout), the per-object stage arguments (ode_obj_args) and the
// copy the host waits for (ode_copy_sync). On the device the two fused attempt kernels share ode_attempt_to_lds and
// the two per-object attempt kernels ode_obj_rows_to_lds; the stage bodies stay four, one per translation unit's
// trunk (the files' headers say why).
#pragma once
#include <cmath>
#include <cstdlib>
#include <functional>
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

// The tableau and the K slots of a fused attempt (ode_attempt_kernel, ode_energy_attempt_kernel) into LDS: read per
// use (wave-uniform), not held in registers across the six stages. tab: 42 doubles (A, then B); the caller's
// barrier follows.
__device__ __forceinline__ void ode_attempt_to_lds(const OdeStageArgs& a, const OdeCtl* c, const OdeTableau& tb,
                                                   double* tab, const double** kin) {
    const int tid = threadIdx.x;
    if (tid < 36) tab[tid] = tb.A[tid];
    else if (tid < 42) tab[tid] = tb.B[tid - 36];
    else if (tid < 42 + ODE_NK) kin[tid - 42] = a.kbuf[c->kidx[tid - 42]];
}

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

// The prologue of a per-object attempt kernel (ode_obj_attempt_kernel, like_obj_attempt_kernel; Args: OdeObjArgs or
// LikeObjArgs), one thread per row of the tile, tableau entry and K slot: the row's object (TANGENT: again at
// obj[ROWS + row], for the likelihood's tangent columns), active / pending flags and step from its record, the tableau
// (all ones for a single evaluation) and the K slots into LDS. Returns whether any row of the workgroup runs (a
// barrier).
template <int ROWS, bool TANGENT, typename Args>
__device__ __forceinline__ int ode_obj_rows_to_lds(const Args& a, const OdeTableau& tb, int r0, int* obj, int* ract,
                                                   int* rpend, double* rh, double* tab, const double** kin) {
    const int tid = threadIdx.x;
    int act = 0;
    if (tid < ROWS) {
        const int o = obj_of_row(r0 + tid, a.rows, a.kper);
        const OdeObjRec* rc = a.rec + o;
        act = (r0 + tid < a.rows) && rc->active != 0;
        obj[tid] = o;
        if (TANGENT) obj[ROWS + tid] = o;
        ract[tid] = act;
        rpend[tid] = rc->pend;
        rh[tid] = rc->h;
    } else if (tid < ROWS + 36) {
        tab[tid - ROWS] = a.single ? 1.0 : tb.A[tid - ROWS];
    } else if (tid < ROWS + 42) {
        tab[tid - ROWS] = tb.B[tid - ROWS - 36];
    } else if (tid < ROWS + 42 + ODE_NK) {
        kin[tid - ROWS - 42] = a.k[tid - ROWS - 42];
    }
    return __syncthreads_or(act);
}

// select_initial_step norms of every object (scipy _ivp/common.py) over its kper rows of NE entries, one wave per
// object: scale = atol + |y0| rtol; f1 == NULL: out[3 b] = rms(y0 / scale), out[3 b + 1] = rms(f0 / scale); else
// out[3 b + 2] = rms((f1 - f0) / scale). A row's squares are added in entry order, the rows by ode_obj_wave_sum.
// NE 9: the sampler's (R,9) state; NE 10: the likelihood's [x (9 R) | logp (R)], a row's logp its tenth entry.
template <int NE>
__global__ __launch_bounds__(64) void ode_obj_init_norms_kernel(const double* __restrict__ y0,
                                                                const double* __restrict__ f0,
                                                                const double* __restrict__ f1, int rows, int kper,
                                                                double atol, double rtol, double* __restrict__ out) {
#pragma clang fp contract(off)
    static_assert(NE == 9 || NE == 10, "nine pose entries, or those and logp");
    const int b = blockIdx.x;
    const size_t n9 = (size_t)rows * 9;
    auto row = [&](int j, int which) {
        const size_t r = (size_t)b * kper + j;
        double sq = 0.0;
        for (int o = 0; o < NE; ++o) {
            const size_t e = o < 9 ? r * 9 + o : n9 + r;
            const double sc = atol + fabs(y0[e]) * rtol;
            const double v = which == 0 ? y0[e] / sc : (which == 1 ? f0[e] / sc : (f1[e] - f0[e]) / sc);
            sq = o == 0 ? v * v : sq + v * v;
        }
        return sq;
    };
    const double rn = sqrt((double)kper * (double)NE);
    if (f1 == nullptr) {
        const double s0 = ode_obj_wave_sum(kper, [&](int j) { return row(j, 0); });
        const double s1 = ode_obj_wave_sum(kper, [&](int j) { return row(j, 1); });
        if (threadIdx.x == 0) {
            out[3 * b] = sqrt(s0) / rn;
            out[3 * b + 1] = sqrt(s1) / rn;
        }
    } else {
        const double s2 = ode_obj_wave_sum(kper, [&](int j) { return row(j, 2); });
        if (threadIdx.x == 0) out[3 * b + 2] = sqrt(s2) / rn;
    }
}

// ------------------------------------------------------------------------------ host constants and status reads
// (the whole-solve entries: gp_ode.hip's, and gp_like_object.hip's through ode_obj_solve)
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

static inline OdeTableau ode_tableau(const double* A = kA6, const double* B = kB6) {
    OdeTableau tb;
    for (int j = 0; j < 36; ++j) tb.A[j] = A[j];
    for (int j = 0; j < 6; ++j) tb.B[j] = B[j];
    return tb;
}

// select_initial_step's host scalars (scipy _ivp/common.py), one definition for every whole-solve entry: they decide
// the first step and with it every later accept and reject, so the order of the float64 operations is fixed.
// -(0.5 g^2) of f(t0): solve_ivp hands t0 as a Python float, so ode_func's g is float32 sigma * float64 scale
static inline double ode_coef_t0(float t32, double dscale) {
    const double g = (double)sigma32(t32) * dscale;
    return -(0.5 * (g * g));
}
// -(0.5 g^2) of every later time: a NumPy float64 t
static inline double ode_coef(double t, double dscale) {
    const double g = kSigMin * pow(kBase, t) * dscale;
    return -(0.5 * (g * g));
}
// the first guess from d0 = rms(y0 / scale), d1 = rms(f0 / scale)
static inline double ode_init_h0(double d0, double d1, double interval) {
    const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    return fmin(h0, interval);
}
// the first step size; d2_raw = rms((f1 - f0) / scale), not yet divided by h0
static inline double ode_init_h_abs(double h0, double d1, double d2_raw, double interval) {
    const double d2 = d2_raw / h0;
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : pow(0.01 / fmax(d1, d2), 1.0 / 5.0);
    return fmin(fmin(100 * h0, h1), interval);
}

static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// The state block every whole-solve workspace starts with: y, y_new, K_0..K_6 and f1 (the Euler probe's
// derivative), each a 256-aligned vector of rows * entries doubles; byte offsets from the base
struct OdeStateBlock {
    size_t y, ynew, k[ODE_NK], f1;
};
static inline OdeStateBlock ode_state_layout(size_t& off, int rows, int entries) {
    OdeStateBlock S = {};
    const size_t vec = align256((size_t)rows * (size_t)entries * sizeof(double));
    S.y = off; off += vec;
    S.ynew = off; off += vec;
    for (int j = 0; j < ODE_NK; ++j) { S.k[j] = off; off += vec; }
    S.f1 = off; off += vec;
    return S;
}

// A copy the host waits for (the whole-solve entries' norm reads and record uploads): `who`: `what` on failure
static inline int ode_copy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t stream,
                                const char* who, const char* what) {
    GP_REQUIRE(hipMemcpyAsync(dst, src, bytes, kind, stream) == hipSuccess &&
                   hipStreamSynchronize(stream) == hipSuccess, "%s: %s", who, what);
    return GP_OK;
}

// The final denoise's scalars of eps (samplers.py:240-249): g is formed from a float32 1-element tensor, so sigma
// and g^2 are float32 products; the step is a float64 quotient rounded once
struct OdeDenoiseScalars {
    float te, sig, g2, step;
};
static inline OdeDenoiseScalars ode_denoise_scalars(double eps, int steps) {
    const float te = (float)eps;
    const float sig = sigma32(te);
    const float g = sig * (float)diff_scale();
    const float step = (float)((1.0 - eps) / (steps > 0 ? steps : 1000));
    return {te, sig, g * g, step};
}

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
    // The four pinned words as the device addresses them, set to -1, or null when it cannot (zc_switch: or when
    // GENPOSE2_ODE_ZC=0 asks for the event-and-copy form)
    int* map(bool zc_switch) {
        const char* zc = zc_switch ? getenv("GENPOSE2_ODE_ZC") : nullptr;
        int* dev = nullptr;
        if ((zc != nullptr && zc[0] == '0') ||
            hipHostGetDevicePointer(reinterpret_cast<void**>(&dev), r.pinned, 0) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        if (dev != nullptr)
            for (int i = 0; i < 4; ++i) const_cast<volatile int*>(r.pinned)[i] = -1;
        return dev;
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

// One right-hand side for gp_ode_rhs, gp_like_rhs and gp_ode_rhs_energy (`who`: the entry's name in messages; its
// own extra checks come first, in the entry): the common checks, the stage arguments, the time row of t32 and
// launch(args), the entry's stage launch, which returns a status.
template <typename Launch>
static inline int ode_rhs_once(const char* who, const gp_head_weights* w, const float* pobj, float t32, float sigma,
                               double coef, const double* y, const double* const* kin, const double* acoef, int nk,
                               double h, int rows, int k, double* kout, void* workspace, size_t workspace_bytes,
                               hipStream_t stream, Launch launch) {
    GP_REQUIRE(w && pobj && y && kout && workspace && rows >= 1 && k >= 1, "%s: bad arguments", who);
    GP_REQUIRE(nk >= 0 && nk < ODE_NK && (nk == 0 || (kin && acoef)), "%s: nk must be in [0, 6]", who);
    GP_REQUIRE(workspace_bytes >= gp_ode_workspace_size(rows), "%s: workspace too small", who);
    OdeStageArgs a = {};
    a.w = *w;
    a.pobj = pobj;
    a.tproj = static_cast<const float*>(workspace);
    a.sigma = sigma;
    a.coef = coef;
    a.y = y;
    for (int j = 0; j < nk; ++j) {
        GP_REQUIRE(kin[j] != nullptr, "%s: null stage pointer", who);
        a.k[j] = kin[j];
        a.a[j] = acoef[j];
    }
    a.nk = nk;
    a.h = h;
    a.kout = kout;
    a.rows = rows;
    a.kper = k;
    GP_TRY(ode_launch_times(w, &t32, 1, workspace, stream));
    return launch(a);
}

// Stages 1..6 of one attempt, in stream order: K_s = f(t + c_s h, y + (sum_{j<s} A[s][j] K_j) h) for s = 1..5
// (tableau_a: 6x6 row-major), then y_new = y + (sum_{j<6} B_j K_j) h, K_6 = f(t + h, y_new) and the error partials.
// set(a, s): the stage's own fields (the host's time row, sigma, coef and K slot, or only a.stage where the
// controller's record supplies them); launch(a, last): the entry's stage launch, which returns a status.
template <typename Set, typename Launch>
static inline int ode_run_stages(OdeStageArgs& a, const double* tableau_a, const double* b, const double* e,
                                 double* ynew, double* part, Set set, Launch launch) {
    for (int s = 1; s < 6; ++s) {
        set(a, s);
        a.nk = s;
        for (int j = 0; j < s; ++j) a.a[j] = tableau_a[s * 6 + j];
        GP_TRY(launch(a, false));
    }
    set(a, 6);
    a.nk = 6;
    for (int j = 0; j < 6; ++j) a.a[j] = b[j];
    for (int j = 0; j < ODE_NK; ++j) a.e[j] = e[j];
    a.ynew = ynew;
    a.part = part;
    return launch(a, true);
}

// One host-controlled attempt for gp_ode_attempt, gp_like_attempt and gp_ode_attempt_energy (`who` as above): the
// common checks, the six time rows, ode_run_stages with the host's scalars and launch(args, last), and the RMS norm
// of the nwg() error partials (the entry's tiling, asked for behind the checks) over `count` elements into err_out.
template <typename Nwg, typename Launch>
static inline int ode_attempt_host(const char* who, const gp_head_weights* w, const float* pobj, const float* t32_6,
                                   const float* sigma_6, const double* coef_6, const double* y, double* const* kslots,
                                   const double* tableau_a, const double* b, const double* e, double h, double rtol,
                                   double atol, int rows, int k, double* ynew, double* err_out, void* workspace,
                                   size_t workspace_bytes, hipStream_t stream, Nwg nwg, double count, Launch launch) {
    GP_REQUIRE(w && pobj && t32_6 && sigma_6 && coef_6 && y && kslots && tableau_a && b && e && ynew && err_out &&
                   workspace && rows >= 1 && k >= 1,
               "%s: bad arguments", who);
    GP_REQUIRE(workspace_bytes >= gp_ode_workspace_size(rows), "%s: workspace too small", who);
    for (int j = 0; j < ODE_NK; ++j) GP_REQUIRE(kslots[j] != nullptr, "%s: null K slot", who);
    const float* tproj = static_cast<const float*>(workspace);
    double* part = reinterpret_cast<double*>(static_cast<char*>(workspace) + ode_part_offset());
    GP_TRY(ode_launch_times(w, t32_6, 6, workspace, stream));
    OdeStageArgs a = {};
    a.w = *w;
    a.pobj = pobj;
    a.y = y;
    a.h = h;
    a.rows = rows;
    a.kper = k;
    a.rtol = rtol;
    a.atol = atol;
    for (int j = 0; j < ODE_NK; ++j) a.k[j] = kslots[j];
    auto set = [&](OdeStageArgs& s, int st) {
        s.tproj = tproj + (size_t)(st - 1) * 768;
        s.sigma = sigma_6[st - 1];
        s.coef = coef_6[st - 1];
        s.kout = kslots[st];
    };
    GP_TRY(ode_run_stages(a, tableau_a, b, e, ynew, part, set, launch));
    return ode_launch_norm(part, nwg(), count, err_out, stream);
}

// The final denoise's common part for gp_ode_denoise / gp_ode_sample_object and gp_ode_denoise_energy: the common
// checks, the time row of t32 and the kernel's arguments into *a
int ode_denoise_begin(const char* who, const gp_head_weights* w, const float* pobj, float t32, float sigma, float g2,
                      float step, const double* x, int rows, int k, const float* pts_center, double* pose, double* q,
                      void* workspace, size_t workspace_bytes, hipStream_t stream, OdeDenoiseArgs* a);
// One launch of ode_obj_control_kernel (the per-object controller: decides attempt n - 1 from the rows' error sums,
// prepares attempt n and its ns folded time rows), as gp_ode_sample_object launches it
int ode_obj_launch_control(const gp_head_weights* w, const float* pobj, const OdeObjRec* cin, OdeObjRec* cout,
                           const double* rowsq, int decide, int prepare, int ns, const OdeConsts& kc, int kper, int nobj,
                           float* init, unsigned long long* count, int* hstat, int* dstat, int n, hipStream_t stream);
// p[0..n) = v (ode_obj_fill_kernel: the row of -0.0f)
int ode_obj_launch_fill(float* p, int n, float v, hipStream_t stream);

// What the workspaces of the per-object entries end in: the controller's buffers, byte offsets from the base
struct OdeObjTail {
    size_t rowsq, norms, rec, init, zrow, count, dstat;
};
static inline OdeObjTail ode_obj_tail_layout(size_t& off, int rows, int nobj) {
    OdeObjTail T = {};
    T.rowsq = off; off += align256((size_t)rows * sizeof(double));
    T.norms = off; off += align256((size_t)nobj * 3 * sizeof(double));
    T.rec = off; off += align256((size_t)nobj * 2 * sizeof(OdeObjRec));
    T.init = off; off += align256((size_t)nobj * 6 * 768 * sizeof(float));
    T.zrow = off; off += align256(768 * sizeof(float));
    T.count = off; off += 256;
    T.dstat = off; off += 256;
    return T;
}

// What the per-object stage arguments share (OdeObjArgs, gp_ode.hip; LikeObjArgs, gp_like_object.hip: the same
// fields and eps), but for the records and `single`. f1: null where only attempts run
template <typename Args>
static inline Args ode_obj_args(const gp_head_weights* w, const float* init, const float* zrow, double* y, double* ynew,
                                double* const* kslots, double* f1, double* rowsq, double rtol, double atol, int rows,
                                int k) {
    Args a = {};
    a.w = *w;
    a.init = init;
    a.zrow = zrow;
    a.y = y;
    a.ynew = ynew;
    for (int j = 0; j < ODE_NK; ++j) {
        a.k[j] = kslots[j];
        a.e[j] = kE7[j];
    }
    a.f1 = f1;
    a.rowsq = rowsq;
    a.rtol = rtol;
    a.atol = atol;
    a.rows = rows;
    a.kper = k;
    a.nobj = rows / k;
    return a;
}

// One per-object solve (ode_obj_solve): nobj objects of k rows with `entries` state entries per row
struct OdeObjSolve {
    const gp_head_weights* w;
    const float* pobj;
    int nobj, k, entries;         // entries: 9 (pose), 10 (pose and logp): every norm runs over k * entries
    double t0, t_bound, rtol, atol;
    OdeObjRec* rec;               // rec[parity * nobj + b]
    float* init;                  // (6, nobj, 768) folded rows
    float* zrow;                  // (768), filled with -0.0f here
    unsigned long long* count;
    int* dstat;
    double* norms;                // (nobj, 3)
    double* rowsq;                // (rows) the stages' error sums
    hipStream_t stream;
    const char* who;              // the entry's name in messages
    OdeObjSolve(const gp_head_weights* w_, const float* pobj_, int nobj_, int k_, int entries_, double t0_,
                double t_bound_, double rtol_, double atol_, char* ws, const OdeObjTail& T, hipStream_t stream_,
                const char* who_)
        : w(w_), pobj(pobj_), nobj(nobj_), k(k_), entries(entries_), t0(t0_), t_bound(t_bound_), rtol(rtol_),
          atol(atol_), rec(reinterpret_cast<OdeObjRec*>(ws + T.rec)), init(reinterpret_cast<float*>(ws + T.init)),
          zrow(reinterpret_cast<float*>(ws + T.zrow)), count(reinterpret_cast<unsigned long long*>(ws + T.count)),
          dstat(reinterpret_cast<int*>(ws + T.dstat)), norms(reinterpret_cast<double*>(ws + T.norms)),
          rowsq(reinterpret_cast<double*>(ws + T.rowsq)), stream(stream_), who(who_) {}
};
// The solve of every object from "the state is in y" to "the final records are on the host": the row of -0.0f and
// the counter, select_initial_step per object (two rounds of host-built records: upload, the slot-0 rows, one
// evaluation, the norms, a read-back), the attempts kept one ahead of the status read (polled pinned words, or a
// 4-byte copy and an event), and the read of the final records: *fin the device's; from the host's copy
// status_out / nfev_out (nobj each) and *failed, whether a solve ended below the spacing of t (each may be null).
// stages(rec, single): the entry's stage kernel on these records (single 0: an attempt; 1: K_0 = f(t, y);
// 2: f1 = f(t, y + K_0 h)); init_norms(with_f1): its ode_obj_init_norms_kernel launch into s.norms.
int ode_obj_solve(const OdeObjSolve& s, const std::function<int(const OdeObjRec*, int)>& stages,
                  const std::function<int(bool)>& init_norms, const OdeObjRec** fin, int* status_out, int* nfev_out,
                  bool* failed);

// ------------------------------------------------------------------------------ host side, gp_ode_energy.hip
// The energy agent's stages: 16-row tiles, exact fp32. Each returns gp_check_launch's status.
bool ode_energy_weights_ok(const gp_head_grad_weights* gw);
int ode_energy_launch_stage(const OdeStageArgs& a, const gp_head_grad_weights& gw, bool last, hipStream_t stream);
int ode_energy_launch_attempt(const OdeStageArgs& a, const gp_head_grad_weights& gw, const OdeTableau& tb,
                              hipStream_t stream);
