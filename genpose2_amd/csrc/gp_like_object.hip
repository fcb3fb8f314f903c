// Per-object likelihood (gp_like_sample_object): cond_ode_likelihood (samplers.py:25-110) as the reference runs it
// when called once per object on that object's k poses. Every object has its own solve_ivp over
// [x_b (9 k) | logp_b (k)] from t0 to t_bound: its own select_initial_step, step controller, stage times, accept /
// reject and nfev, its RMS norms over its own 10 k entries, so its result does not depend on which other objects
// share the call.
//
// The per-object machinery is gp_ode_sample_object's, and the solve itself is the same host driver (ode_obj_solve,
// gp_ode.hip) with this file's stage launch: one OdeObjRec per object, decided and prepared by
// ode_obj_control_kernel (the norm's count is 10 k here, the direction +1), the folded rows
// init[s][b] = pobj[b] + tproj(t32[b][s]) and the row of -0.0f in place of the trunk's pobj and tproj, the status
// words and their poll. What differs is the stage: like_obj_attempt_kernel carries the JVP trunk of
// like_stage_kernel (NP primal column tiles and their NP tangent tiles; the tangent columns see no pobj / tproj
// term), the state is scipy's flat [x (9 R) | logp (R)] of the call's R rows, and a row's error sum covers its ten
// entries in entry order (nine x, then logp). The attempt kernel's row-record prologue (ode_obj_rows_to_lds), the
// workspace's state block (ode_state_layout) and the common stage arguments (ode_obj_args) are gp_ode.h's, shared
// with gp_ode_sample_object. These kernels have a translation unit of their own so that they
// cannot move the register assignment of the kernels that were there before them.
#include <cstddef>

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
    // none of this workgroup's objects runs: done
    if (!ode_obj_rows_to_lds<ROWS, true>(a, tb, r0, obj, ract, rpend, rh, tab, kin)) return;
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
    OdeStateBlock st;
    size_t dlogp, total;
    OdeObjTail tail;
};
LikeObjLayout like_obj_layout(int rows, int nobj) {
    LikeObjLayout L = {};
    size_t off = 0;
    L.st = ode_state_layout(off, rows, 10);
    L.dlogp = off; off += align256((size_t)rows * sizeof(double));
    L.tail = ode_obj_tail_layout(off, rows, nobj);
    L.total = off;
    return L;
}

// Primal column tiles per workgroup: like_stage_kernel's rule (gp_ode.hip like_np) on the whole batch's rows
int like_obj_np(const gp_head_weights* w, int rows_total) {
    return (w->pe2_h != nullptr && rows_total >= PC_SPLIT_NT2_MIN) ? 2 : 1;
}

// The stage arguments but for the records and `single` (f1: null where only attempts run)
LikeObjArgs like_obj_args(const gp_head_weights* w, const float* init, const float* zrow, const float* eps, double* y,
                          double* ynew, double* const* kslots, double* f1, double* rowsq, double rtol, double atol,
                          int rows, int k) {
    LikeObjArgs a = ode_obj_args<LikeObjArgs>(w, init, zrow, y, ynew, kslots, f1, rowsq, rtol, atol, rows, k);
    a.eps = eps;
    return a;
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
    char* ws = static_cast<char*>(workspace);
    auto dptr = [&](size_t off) { return reinterpret_cast<double*>(ws + off); };
    const OdeObjSolve sv(w, pobj, nobj, k, 10, t0, t_bound, rtol, atol, ws, L.tail, stream, "like_sample_object");
    const long long n9 = (long long)rows * 9, n = (long long)rows * 10;
    const int np = like_obj_np(w, rows_total);   // the whole batch's tile class
    double* K[ODE_NK];
    for (int j = 0; j < ODE_NK; ++j) K[j] = dptr(L.st.k[j]);
    LikeObjArgs a = like_obj_args(w, sv.init, sv.zrow, eps_dir, dptr(L.st.y), dptr(L.st.ynew), K, dptr(L.st.f1),
                                  sv.rowsq, rtol, atol, rows, k);
    const OdeTableau tb = ode_tableau();
    auto stages = [&](const OdeObjRec* r, int single) {
        a.rec = r;
        a.single = single;
        return like_obj_launch(a, tb, np, stream);
    };
    auto init_norms = [&](bool with_f1) {
        hipLaunchKernelGGL(ode_obj_init_norms_kernel<10>, dim3(nobj), dim3(64), 0, stream, (const double*)a.y,
                           (const double*)a.k[0], (const double*)(with_f1 ? a.f1 : nullptr), rows, k, atol, rtol,
                           sv.norms);
        return gp_check_launch("ode_obj_init_norms_kernel");
    };
    int rc;
    hipLaunchKernelGGL(like_obj_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, a.y, n9, n);
    if ((rc = gp_check_launch("like_obj_state_kernel"))) return rc;
    const OdeObjRec* fin = nullptr;
    if ((rc = ode_obj_solve(sv, stages, init_norms, &fin, status_out, nfev_out, nullptr))) return rc;
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
    LikeObjArgs a = like_obj_args(w, init, zrow, eps_dir, y, ynew, kslots, nullptr, rowsq, rtol, atol, rows, k);
    a.rec = r;
    return like_obj_launch(a, ode_tableau(), like_obj_np(w, rows_total), stream);
}
