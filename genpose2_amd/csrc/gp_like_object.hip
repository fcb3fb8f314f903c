// Per-object likelihood (gp_like_sample_object): cond_ode_likelihood (samplers.py:25-110) as the reference runs it
// when called once per object on that object's k poses. Every object has its own solve_ivp over
// [x_b (9 k) | logp_b (k)] from t0 to t_bound: its own select_initial_step, step controller, stage times, accept /
// reject and nfev, its RMS norms over its own 10 k entries, so its result does not depend on which other objects
// share the call.
//
// The per-object machinery is gp_ode_sample_object's (gp_ode.hip): one OdeObjRec per object, decided and prepared
// by ode_obj_control_kernel (unchanged: the norm's count is 10 k here, the direction +1), the folded rows
// init[s][b] = pobj[b] + tproj(t32[b][s]) and the row of -0.0f in place of the trunk's pobj and tproj, the status
// words and their poll. What differs is the stage: like_obj_attempt_kernel carries the JVP trunk of
// like_stage_kernel (NP primal column tiles and their NP tangent tiles; the tangent columns see no pobj / tproj
// term), the state is scipy's flat [x (9 R) | logp (R)] of the call's R rows, and a row's error sum covers its ten
// entries in entry order (nine x, then logp). These kernels have a translation unit of their own so that they
// cannot move the register assignment of the kernels that were there before them.
#include <chrono>
#include <cstddef>
#include <cstdlib>
#include <vector>

#include "gp_ode.h"

struct LikeObjArgs {
    gp_head_weights w;
    const float* init;            // (6, nobj, 768) folded rows of the prepared attempt
    const float* zrow;            // (768) of -0.0f
    const OdeObjRec* rec;         // (nobj) records of the prepared attempt
    const float* eps;             // (R,9) Skilling-Hutchinson direction, constant over the solve
    double* y;                    // (10 R) state at the step's start: x (R,9), then logp (R)
    double* ynew;                 // (10 R) the attempt's end
    double* k[ODE_NK];            // K_0..K_6, fixed slots, the state's layout
    double* f1;                   // (10 R) the Euler probe's derivative (select_initial_step)
    double* rowsq;                // (R) sum over a row's 10 entries of (err/scale)^2, in increasing entry order
    double e[ODE_NK];
    double rtol, atol;
    int rows, kper, nobj;
    int single;                   // 0: an attempt; 1: K_0 = f(t, y); 2: f1 = f(t, y + K_0 h) (both with slot 0's row)
};

// The six stages of every object's attempt in one launch, with the tiling of the whole batch (NP of rows_total):
// like_stage_kernel's stage with h, coef, sigma and active / inactive per row, from the row's object record. A
// workgroup without an active row returns at once. The workgroup that owns an accepted object's rows copies
// y_new -> y and K_6 -> K_0 (FSAL) in the next attempt's prologue, and only when that object runs again: a finished
// object's buffers are never written again.
// The stages are iterations of one loop around one trunk call in the kernel's own body, as like_stage_kernel calls
// it: the exact-fp32 JVP trunk's layer-2 sums are not under contract(off), and behind a stage function the compiler
// contracted other products of them than in like_stage_kernel (gp_head.h run_head_trunk has the same finding).
template <int PL, int NP>
__global__ __launch_bounds__(EVAL_WV * 64) void like_obj_attempt_kernel(LikeObjArgs a, OdeTableau tb) {
    constexpr int NT = 2 * NP;
    constexpr int ROWS = 16 * NP;     // rows (poses) of this workgroup
    constexpr int NTH = EVAL_WV * 64;
    static_assert(ROWS + 42 + ODE_NK <= NTH, "one thread per row, tableau entry and K slot");
    __shared__ HeadSmem<NT, EVAL_WV, PL> sm;
    __shared__ int obj[2 * ROWS], ract[ROWS], rpend[ROWS];   // obj: the primal columns' objects, again for the tangents
    __shared__ double rh[ROWS], rcoef[ROWS];
    __shared__ float rsig[ROWS];
    __shared__ double y0s[ROWS * 10], y1s[ROWS * 10];
    __shared__ double tab[42];
    __shared__ const double* kin[ODE_NK];
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * ROWS;
    const size_t n9 = (size_t)a.rows * 9;
    int act = 0;
    if (tid < ROWS) {
        const int o = obj_of_row(r0 + tid, a.rows, a.kper);
        const OdeObjRec* rc = a.rec + o;
        act = (r0 + tid < a.rows) && rc->active != 0;
        obj[tid] = o;
        obj[ROWS + tid] = o;
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
    if (!__syncthreads_or(act)) return;   // none of this workgroup's objects runs
    if (!a.single) {
        // the accepted step of the objects that go on: y_new -> y, K_6 -> K_0 (these rows are this workgroup's in
        // every attempt; the first stage's barrier orders the stores before the stages' loads)
        for (int e10 = tid; e10 < ROWS * 10; e10 += NTH) {
            const int c = e10 / 10, o = e10 - c * 10;
            if (ract[c] && rpend[c]) {
                const size_t e = o < 9 ? (size_t)(r0 + c) * 9 + o : n9 + (size_t)(r0 + c);
                a.y[e] = a.ynew[e];
                a.k[0][e] = a.k[ODE_NK - 1][e];
            }
        }
    }
    // an attempt: stages s = 1..6 (stage 6: B, y_new and the rows' error sums); single: the one evaluation
    const int s_end = a.single ? 1 : 6;
    for (int s = 1; s <= s_end; ++s) {
        __syncthreads();   // the copies above; stage s-1's K stores and its reads of the staged weights are done
        const bool last = !a.single && s == 6;
        const int nk = a.single ? a.single - 1 : s;           // y_in = y + (sum_{j<nk} acoef_j K_j) h
        const int slot = a.single ? 0 : s - 1;                // which of the prepared rows and scalars
        const double* acoef = a.single ? tab : tab + (last ? 36 : s * 6);
        double* kout = a.single ? (a.single == 1 ? a.k[0] : a.f1) : a.k[s];
        // per stage (L2-resident): held across the stages they would add to the trunk's register peak
        const SplitScalars hs = load_split_scalars<PL>(a.w);
        stage_small_weights(a.w, sm);
        for (int i = tid; i < 2 * ROWS * 16; i += NTH) {
            const int c = i >> 4, j = i & 15;
            float xv = 0.f;
            if (c < ROWS) {
                const int r = r0 + c;
                if (r < a.rows && j < 9 && ract[c]) {
                    const size_t e = (size_t)r * 9 + j;
                    const double yv = a.y[e];
                    const double yi = nk > 0 ? ode_stage_in(kin, acoef, nk, rh[c], e, yv) : yv;
                    xv = (float)yi;   // torch.tensor(x, dtype=torch.float32) (samplers.py:83)
                    if (last) {
                        y0s[c * 10 + j] = yv;
                        y1s[c * 10 + j] = yi;
                        a.ynew[e] = yi;
                    }
                }
            } else {
                const int r = r0 + c - ROWS;
                if (r < a.rows && j < 9 && ract[c - ROWS]) xv = a.eps[(size_t)r * 9 + j];
            }
            sm.xin[i] = xv;
        }
        if (last && tid < ROWS && r0 + tid < a.rows && ract[tid]) {   // logp: only in y_new and the error
            const size_t e = n9 + (size_t)(r0 + tid);
            const double yv = a.y[e];
            const double yi = ode_stage_in(kin, acoef, nk, rh[tid], e, yv);
            y0s[tid * 10 + 9] = yv;
            y1s[tid * 10 + 9] = yi;
            a.ynew[e] = yi;
        }
        if (tid < ROWS) {
            const OdeObjRec* rc = a.rec + obj[tid];
            rcoef[tid] = rc->coef[slot];
            rsig[tid] = rc->sig[slot];
        }
        // the folded rows pobj[b] + tproj(t32[b][slot]) as the trunk's pobj, the row of -0.0f as its tproj
        const float* prow = a.init + (size_t)slot * a.nobj * 768;
        if constexpr (PL != 0)
            head_trunk_x3<NT, EVAL_WV, false, true>(a.w, prow, a.zrow, obj, sm, 0, hs);
        else
            head_trunk<NT, EVAL_WV, true>(a.w, prow, a.zrow, obj, sm);
        for (int e10 = tid; e10 < ROWS * 10; e10 += NTH) {
#pragma clang fp contract(off)
            const int c = e10 / 10, o = e10 - c * 10;
            const int r = r0 + c;
            if (r < a.rows && ract[c]) {
                const size_t e = o < 9 ? (size_t)r * 9 + o : n9 + (size_t)r;
                const float den = fadd(rsig[c], 1e-7f);
                float sv;
                if (o < 9) {
                    sv = fdiv(head_out(sm, c, o), den);
                } else {   // eps . (J eps): nine fp32 products, each rounded on its own, summed in order
                    sv = 0.f;
#pragma unroll
                    for (int j = 0; j < 9; ++j)
                        sv = fadd(sv, fmul(ld1(&sm.xin[(ROWS + c) * 16 + j]), fdiv(head_out<true>(sm, ROWS + c, j), den)));
                }
                const double kv = rcoef[c] * (double)sv;
                kout[e] = kv;
                if (last) {
                    const double er = ode_err_term(a, kin, kv, rh[c], e, y0s[e10], y1s[e10]);
                    y1s[e10] = er * er;   // its own entry: read above by this thread only
                }
            }
        }
        if (last) {   // a row's ten squares in entry order (nine x, then logp)
            __syncthreads();
            if (tid < ROWS && r0 + tid < a.rows && ract[tid]) {
#pragma clang fp contract(off)
                double sq = y1s[tid * 10];
                for (int o = 1; o < 10; ++o) sq += y1s[tid * 10 + o];
                a.rowsq[r0 + tid] = sq;
            }
        }
    }
}

// select_initial_step norms of every object (scipy _ivp/common.py) over its 10 k entries, one wave per object:
// ode_obj_init_norms_kernel with a row's ten entries (nine x, then logp) in entry order, the rows by
// ode_obj_wave_sum. f1 == NULL: out[3 b] = rms(y0 / scale), out[3 b + 1] = rms(f0 / scale); else
// out[3 b + 2] = rms((f1 - f0) / scale); scale = atol + |y0| rtol.
__global__ __launch_bounds__(64) void like_obj_init_norms_kernel(const double* __restrict__ y0,
                                                                 const double* __restrict__ f0,
                                                                 const double* __restrict__ f1, int rows, int kper,
                                                                 double atol, double rtol, double* __restrict__ out) {
#pragma clang fp contract(off)
    const int b = blockIdx.x;
    const size_t n9 = (size_t)rows * 9;
    auto row = [&](int j, int which) {
        const size_t r = (size_t)b * kper + j;
        double sq = 0.0;
        for (int o = 0; o < 10; ++o) {
            const size_t e = o < 9 ? r * 9 + o : n9 + r;
            const double sc = atol + fabs(y0[e]) * rtol;
            const double v = which == 0 ? y0[e] / sc : (which == 1 ? f0[e] / sc : (f1[e] - f0[e]) / sc);
            sq = o == 0 ? v * v : sq + v * v;
        }
        return sq;
    };
    const double rn = sqrt((double)kper * 10.0);
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

// y = [float64(x) (9 R) | init_logp = 0 (R)] (samplers.py:92)
__global__ __launch_bounds__(256) void like_obj_state_kernel(const float* __restrict__ x, double* __restrict__ y,
                                                             long long n9, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = i < n9 ? (double)x[i] : 0.0;
}

// res.y[:, -1] of every object (its state is in y_new while the accepted step is not copied, else in y) and the
// likelihood in bits (samplers.py:100-109): z (R,9), delta_logp (R), and
// ll = (prior_logp(z) + delta_logp) / ln 2, prior_logp = log_term - sum(z^2) / two_sig2 (global_prior_likelihood,
// samplers.py:14-22), in float64 with the reference's float32 scalars; a row's nine squares are added in entry order.
struct LikeObjFinalArgs {
    const OdeObjRec* rec;
    const double* y;
    const double* ynew;
    double log_term, two_sig2, ln2;
    int rows, kper;
    double* z;
    double* dlogp;
    double* ll;
};
__global__ __launch_bounds__(256) void like_obj_final_kernel(LikeObjFinalArgs a) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.rows) return;
    const double* src = a.rec[r / a.kper].pend ? a.ynew : a.y;
    double ss = 0.0;
    for (int o = 0; o < 9; ++o) {
        const double v = src[(size_t)r * 9 + o];
        a.z[(size_t)r * 9 + o] = v;
        ss = o == 0 ? v * v : ss + v * v;
    }
    const double dl = src[(size_t)a.rows * 9 + r];
    a.dlogp[r] = dl;
    a.ll[r] = ((a.log_term - ss / a.two_sig2) + dl) / a.ln2;
}

namespace {
struct LikeObjLayout {
    size_t y, ynew, k[ODE_NK], f1, dlogp, rowsq, norms, rec, init, zrow, count, dstat, total;
};
LikeObjLayout like_obj_layout(int rows, int nobj) {
    LikeObjLayout L = {};
    const size_t vec = align256((size_t)rows * 10 * sizeof(double));
    const size_t rowv = align256((size_t)rows * sizeof(double));
    size_t off = 0;
    L.y = off; off += vec;
    L.ynew = off; off += vec;
    for (int j = 0; j < ODE_NK; ++j) { L.k[j] = off; off += vec; }
    L.f1 = off; off += vec;
    L.dlogp = off; off += rowv;
    L.rowsq = off; off += rowv;
    L.norms = off; off += align256((size_t)nobj * 3 * sizeof(double));
    L.rec = off; off += align256((size_t)nobj * 2 * sizeof(OdeObjRec));
    L.init = off; off += align256((size_t)nobj * 6 * 768 * sizeof(float));
    L.zrow = off; off += align256(768 * sizeof(float));
    L.count = off; off += 256;
    L.dstat = off; off += 256;
    L.total = off;
    return L;
}

// Primal column tiles per workgroup: like_stage_kernel's rule (gp_ode.hip like_np) on the whole batch's rows
int like_obj_np(const gp_head_weights* w, int rows_total) {
    return (w->pe2_h != nullptr && rows_total >= PC_SPLIT_NT2_MIN) ? 2 : 1;
}

int like_obj_launch(const LikeObjArgs& a, const OdeTableau& tb, int np, hipStream_t stream) {
    const dim3 grid((a.rows + 16 * np - 1) / (16 * np)), blk(EVAL_WV * 64);
    head_dispatch<2>(a.w.pe2_h ? X3P : 0, np, [&](auto pl, auto npc) {
        hipLaunchKernelGGL((like_obj_attempt_kernel<pl.value, npc.value>), grid, blk, 0, stream, a, tb);
    });
    return gp_check_launch("like_obj_attempt_kernel");
}
}  // namespace

extern "C" size_t gp_like_object_workspace_size_k(int rows, int k) {
    return (rows >= 1 && k >= 1 && rows % k == 0) ? like_obj_layout(rows, rows / k).total : 0;
}
// enough for every k (k = 1: one record and six rows per pose)
extern "C" size_t gp_like_object_workspace_size(int rows) { return gp_like_object_workspace_size_k(rows, 1); }

extern "C" int gp_like_sample_object(const gp_head_weights* w, const float* pobj, const float* x, const float* eps_dir,
                                     int rows, int k, int rows_total, double t0, double t_bound, double rtol,
                                     double atol, double* z, double* ll, int* nfev_out, int* status_out,
                                     void* workspace, size_t workspace_bytes, hipStream_t stream) {
    GP_REQUIRE(w && pobj && x && eps_dir && z && ll && nfev_out && status_out && workspace,
               "like_sample_object: null pointer");
    GP_REQUIRE(rows >= 1 && k >= 1, "like_sample_object: bad arguments (rows %d, k %d)", rows, k);
    GP_REQUIRE(rows % k == 0, "like_sample_object: rows %d are not whole objects of k = %d", rows, k);
    GP_REQUIRE(rows_total >= rows && rows_total % k == 0,
               "like_sample_object: rows_total %d must be whole objects and hold this call's %d rows", rows_total,
               rows);
    GP_REQUIRE(t0 != t_bound, "like_sample_object: empty integration interval (t0 == t_bound)");
    const int nobj = rows / k;
    const LikeObjLayout L = like_obj_layout(rows, nobj);
    GP_REQUIRE(workspace_bytes >= L.total,
               "like_sample_object: workspace too small (gp_like_object_workspace_size_k(rows, k))");
    StatusLease status;
    GP_REQUIRE(status.acquire(stream) == 0, "like_sample_object: pinned status word / event");
    char* ws = static_cast<char*>(workspace);
    auto dptr = [&](size_t off) { return reinterpret_cast<double*>(ws + off); };
    OdeObjRec* rec = reinterpret_cast<OdeObjRec*>(ws + L.rec);   // rec[parity * nobj + b]
    float* init = reinterpret_cast<float*>(ws + L.init);
    float* zrow = reinterpret_cast<float*>(ws + L.zrow);
    unsigned long long* count = reinterpret_cast<unsigned long long*>(ws + L.count);
    int* dstat = reinterpret_cast<int*>(ws + L.dstat);
    double* norms = dptr(L.norms);
    const long long n9 = (long long)rows * 9, n = (long long)rows * 10;
    const double tf = t_bound, dir = tf > t0 ? 1.0 : -1.0;
    const double dscale = diff_scale();
    const int np = like_obj_np(w, rows_total);   // the whole batch's tile class
    // every norm of an object runs over its 10 k entries
    const OdeConsts kc = {tf, dir, rtol, atol, kSigMin, kBase, dscale, (double)k * 10.0, 0};

    LikeObjArgs a = {};
    a.w = *w;
    a.init = init;
    a.zrow = zrow;
    a.eps = eps_dir;
    a.y = dptr(L.y);
    a.ynew = dptr(L.ynew);
    for (int j = 0; j < ODE_NK; ++j) {
        a.k[j] = dptr(L.k[j]);
        a.e[j] = kE7[j];
    }
    a.f1 = dptr(L.f1);
    a.rowsq = dptr(L.rowsq);
    a.rtol = rtol;
    a.atol = atol;
    a.rows = rows;
    a.kper = k;
    a.nobj = nobj;
    OdeTableau tb;
    for (int j = 0; j < 36; ++j) tb.A[j] = kA6[j];
    for (int j = 0; j < 6; ++j) tb.B[j] = kB6[j];
    auto stages = [&](const OdeObjRec* r, int single) {
        a.rec = r;
        a.single = single;
        return like_obj_launch(a, tb, np, stream);
    };
    // rows of slot 0 for host-prepared records (the two select_initial_step evaluations)
    auto rows0 = [&](const OdeObjRec* r) {
        return ode_obj_launch_control(w, pobj, r, nullptr, nullptr, 0, 0, 1, kc, k, nobj, init, count, nullptr, dstat, 0,
                                      stream);
    };
    int rc;
    GP_REQUIRE(hipMemsetAsync(count, 0, 256, stream) == hipSuccess, "like_sample_object: counter");
    if ((rc = ode_obj_launch_fill(zrow, 768, -0.0f, stream))) return rc;
    hipLaunchKernelGGL(like_obj_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, a.y, n9, n);
    if ((rc = gp_check_launch("like_obj_state_kernel"))) return rc;

    // ---- select_initial_step (scipy common.py) per object, gp_ode_sample_object's scalar expressions element by
    //      element
    std::vector<OdeObjRec> hrec((size_t)nobj);
    std::vector<double> hn((size_t)nobj * 3);
    auto upload = [&](int parity) {
        return hipMemcpyAsync(rec + (size_t)parity * nobj, hrec.data(), sizeof(OdeObjRec) * (size_t)nobj,
                              hipMemcpyHostToDevice, stream) == hipSuccess &&
               hipStreamSynchronize(stream) == hipSuccess;
    };
    auto norms_back = [&]() {
        return hipMemcpyAsync(hn.data(), norms, sizeof(double) * 3 * (size_t)nobj, hipMemcpyDeviceToHost, stream) ==
                   hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    };
    auto init_norms = [&](const double* f1) {
        hipLaunchKernelGGL(like_obj_init_norms_kernel, dim3(nobj), dim3(64), 0, stream, (const double*)a.y,
                           (const double*)a.k[0], f1, rows, k, atol, rtol, norms);
        return gp_check_launch("like_obj_init_norms_kernel");
    };
    {   // f(t0): solve_ivp hands t0 as a Python float, so ode_func's g is float32 sigma * float64 scale
        const float t32 = (float)t0;
        const double g = (double)sigma32(t32) * dscale;
        for (int b = 0; b < nobj; ++b) {
            OdeObjRec r = {};
            r.t = t0;
            r.active = 1;
            r.t32[0] = t32;
            r.sig[0] = sigma32(t32);
            r.coef[0] = -(0.5 * (g * g));
            hrec[(size_t)b] = r;
        }
    }
    GP_REQUIRE(upload(0), "like_sample_object: records");
    if ((rc = rows0(rec))) return rc;
    if ((rc = stages(rec, 1))) return rc;
    if ((rc = init_norms(nullptr))) return rc;
    GP_REQUIRE(norms_back(), "like_sample_object: norm read");
    const double interval = fabs(tf - t0);
    std::vector<double> h0v((size_t)nobj);
    for (int b = 0; b < nobj; ++b) {
        const double d0 = hn[3 * (size_t)b], d1 = hn[3 * (size_t)b + 1];
        double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
        h0 = fmin(h0, interval);
        h0v[(size_t)b] = h0;
        // f(t0 + h0 dir, y0 + h0 dir f0): a NumPy float64 time from here on
        const double t = t0 + h0 * dir;
        const double g = kSigMin * pow(kBase, t) * dscale;
        OdeObjRec& r = hrec[(size_t)b];
        r.h = h0 * dir;
        r.t32[0] = (float)t;
        r.sig[0] = sigma32((float)t);
        r.coef[0] = -(0.5 * (g * g));
    }
    GP_REQUIRE(upload(1), "like_sample_object: records");
    if ((rc = rows0(rec + nobj))) return rc;
    if ((rc = stages(rec + nobj, 2))) return rc;
    if ((rc = init_norms(a.f1))) return rc;
    GP_REQUIRE(norms_back(), "like_sample_object: norm read");
    for (int b = 0; b < nobj; ++b) {
        const double d1 = hn[3 * (size_t)b + 1], h0 = h0v[(size_t)b];
        const double d2 = hn[3 * (size_t)b + 2] / h0;
        const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : pow(0.01 / fmax(d1, d2), 1.0 / 5.0);
        OdeObjRec r = {};
        r.t = t0;
        r.h_abs = fmin(fmin(100 * h0, h1), interval);
        r.nfev = 2;
        hrec[(size_t)b] = r;
    }
    GP_REQUIRE(upload(0), "like_sample_object: records");

    // ---- the attempts, one enqueued ahead of the status read; the loop ends when no object runs
    int* hs_dev = nullptr;   // the pinned words as the device addresses them, if it can
    {
        const char* zc = getenv("GENPOSE2_ODE_ZC");
        if ((zc != nullptr && zc[0] == '0') ||
            hipHostGetDevicePointer(reinterpret_cast<void**>(&hs_dev), status.r.pinned, 0) != hipSuccess) {
            hs_dev = nullptr;
            (void)hipGetLastError();
        }
    }
    auto control = [&](int at) {   // decides attempt at - 1, prepares attempt at
        return ode_obj_launch_control(w, pobj, rec + (size_t)(at & 1) * nobj, rec + (size_t)((at + 1) & 1) * nobj,
                                      a.rowsq, at > 0 ? 1 : 0, 1, 6, kc, k, nobj, init, count, hs_dev, dstat, at, stream);
    };
    auto attempt = [&](int at) { return stages(rec + (size_t)((at + 1) & 1) * nobj, 0); };
    int at = 0;
    if (hs_dev != nullptr) {
        volatile int* hv = status.r.pinned;
        for (int i = 0; i < 4; ++i) hv[i] = -1;
        status.pending = true;   // the device writes the words until the stream drains
        if ((rc = control(0)) || (rc = attempt(0))) return rc;
        for (;; ++at) {
            GP_REQUIRE(at < 100000, "like_sample_object: attempt limit reached");
            if ((rc = control(at + 1)) || (rc = attempt(at + 1))) return rc;
            const int want = at + 1;
            const auto t_end = std::chrono::steady_clock::now() + std::chrono::seconds(60);
            int v;
            while (((v = hv[want & 3]) >> 2) != want)
                GP_REQUIRE(std::chrono::steady_clock::now() < t_end, "like_sample_object: no status from attempt %d",
                           want);
            if ((v & 3) != 1) break;
        }
    } else {
        if ((rc = control(0)) || (rc = attempt(0))) return rc;
        for (;; ++at) {
            GP_REQUIRE(at < 100000, "like_sample_object: attempt limit reached");
            if ((rc = control(at + 1))) return rc;
            status.pending = true;
            GP_REQUIRE(hipMemcpyAsync(status.r.pinned, dstat, 4, hipMemcpyDeviceToHost, stream) == hipSuccess &&
                           hipEventRecord(status.r.ev, stream) == hipSuccess, "like_sample_object: status read");
            if ((rc = attempt(at + 1))) return rc;   // a no-op once no object runs
            GP_REQUIRE(hipEventSynchronize(status.r.ev) == hipSuccess, "like_sample_object: status wait");
            status.pending = false;
            GP_REQUIRE((*status.r.pinned >> 2) == at + 1, "like_sample_object: status word of attempt %d", at + 1);
            if ((*status.r.pinned & 3) != 1) break;
        }
    }
    const OdeObjRec* fin = rec + (size_t)((at + 2) & 1) * nobj;
    GP_REQUIRE(hipMemcpyAsync(hrec.data(), fin, sizeof(OdeObjRec) * (size_t)nobj, hipMemcpyDeviceToHost, stream) ==
                       hipSuccess && hipStreamSynchronize(stream) == hipSuccess, "like_sample_object: final records");
    status.pending = false;
    for (int b = 0; b < nobj; ++b) {
        status_out[b] = hrec[(size_t)b].status;
        nfev_out[b] = hrec[(size_t)b].nfev;
    }
    // ---- the latent and the likelihood in bits. sigma_max and the log term are float32 scalars in the reference
    //      (sigma(1.0) of a float32 tensor; -9/2 log(2 pi sigma_max^2) in float32), z float64
    LikeObjFinalArgs fa = {};
    fa.rec = fin;
    fa.y = a.y;
    fa.ynew = a.ynew;
    const float smax = sigma32(1.0f), s2 = smax * smax;
    fa.log_term = (double)(-4.5f * logf((float)(2.0 * 3.14159265358979323846) * s2));
    fa.two_sig2 = (double)(2.0f * s2);
    fa.ln2 = log(2.0);
    fa.rows = rows;
    fa.kper = k;
    fa.z = z;
    fa.dlogp = dptr(L.dlogp);
    fa.ll = ll;
    hipLaunchKernelGGL(like_obj_final_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, fa);
    return gp_check_launch("like_obj_final_kernel");
}

// Test aid: one launch of like_obj_attempt_kernel as gp_like_sample_object launches it for an attempt, from
// host-given records on caller-owned device buffers. rec: nobj = rows / k records of gp_debug_ode_obj_rec_size()
// bytes (h, t32[6], sig[6], coef[6], active and pend are read); y, ynew and the seven K slots: 10 rows doubles each
// in the state's layout [x (9 rows) | logp (rows)], K_0 given; rowsq (rows); scratch: (6 nobj + 1) x 768 floats (the
// folded rows, formed here from the records' t32, and the row of -0.0f). Not part of the likelihood's ABI contract.
extern "C" int gp_debug_like_obj_attempt(const gp_head_weights* w, const float* pobj, const void* rec,
                                         const float* eps_dir, double* y, double* ynew, double* const* kslots,
                                         double* rowsq, float* scratch, int rows, int k, int rows_total, double rtol,
                                         double atol, hipStream_t stream) {
    GP_REQUIRE(w && pobj && rec && eps_dir && y && ynew && kslots && rowsq && scratch,
               "debug_like_obj_attempt: null pointer");
    GP_REQUIRE(rows >= 1 && k >= 1 && rows % k == 0 && rows_total >= rows && rows_total % k == 0,
               "debug_like_obj_attempt: rows %d / rows_total %d are not whole objects of k = %d", rows, rows_total, k);
    for (int j = 0; j < ODE_NK; ++j) GP_REQUIRE(kslots[j] != nullptr, "debug_like_obj_attempt: null K slot");
    const int nobj = rows / k;
    float* init = scratch;
    float* zrow = scratch + (size_t)6 * nobj * 768;
    const OdeObjRec* r = static_cast<const OdeObjRec*>(rec);
    const OdeConsts kc = {1.0, 1.0, rtol, atol, kSigMin, kBase, diff_scale(), (double)k * 10.0, 0};
    int rc;
    if ((rc = ode_obj_launch_fill(zrow, 768, -0.0f, stream))) return rc;
    // prepare = 0: only the six folded rows of every active object, from its record's t32
    if ((rc = ode_obj_launch_control(w, pobj, r, nullptr, nullptr, 0, 0, 6, kc, k, nobj, init, nullptr, nullptr, nullptr,
                                     0, stream)))
        return rc;
    LikeObjArgs a = {};
    a.w = *w;
    a.init = init;
    a.zrow = zrow;
    a.rec = r;
    a.eps = eps_dir;
    a.y = y;
    a.ynew = ynew;
    for (int j = 0; j < ODE_NK; ++j) {
        a.k[j] = kslots[j];
        a.e[j] = kE7[j];
    }
    a.rowsq = rowsq;
    a.rtol = rtol;
    a.atol = atol;
    a.rows = rows;
    a.kper = k;
    a.nobj = nobj;
    OdeTableau tb;
    for (int j = 0; j < 36; ++j) tb.A[j] = kA6[j];
    for (int j = 0; j < 6; ++j) tb.B[j] = kB6[j];
    return like_obj_launch(a, tb, like_obj_np(w, rows_total), stream);
}
