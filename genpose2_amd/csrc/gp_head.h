// Shared score-head trunk for gfx950: LDS layout, streamed-weight MFMA layers, and pose helpers.
// Used by the PC sampler / score / energy kernels (gp_score.hip) and the ODE stage kernels
// (gp_ode.hip). Reference: PoseScoreNet.forward (networks/gf_algorithms/scorenet.py:215-275).
#pragma once
#include <type_traits>

#include "gp_common.h"

constexpr int HT = 256;          // threads per workgroup
constexpr int HID = 256;         // pose/head hidden width
constexpr int KG_HID = HID / 16; // k-groups over a 256-wide activation
#ifndef PC_WV1
#define PC_WV1 8                 // waves per workgroup, 16-candidate PC tiles
#endif
#ifndef EVAL_WV
#define EVAL_WV 8                // waves per workgroup, score/energy evaluation
#endif
#ifndef PC_D2
#define PC_D2 3                  // k-groups of pose_encoder.2 weights kept in flight
#endif
#ifndef HEAD_PREFETCH
#define HEAD_PREFETCH 2          // k-groups of head-layer-1 weights kept in flight
#endif


// Phase stamps (PC_MARK) are defined by the including file; no-op by default.
#ifndef PC_MARK
#define PC_MARK(k) ((void)trace_slot)
#endif


// The thread id behind an opaque copy: per-lane values derived from it are computed where they are used and
// cannot be hoisted out of an enclosing loop (a trunk run once per loop iteration kept hoisted lane addresses
// live across every trunk and spilled them, their reloads draining the weight ring)
__device__ __forceinline__ int tid_x() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

// ============================================================================ shared head trunk
// NT = column tiles (16 candidates each) per workgroup. PL = 0: the exact-fp32 trunk's activations
// (fp32, accumulator-native); PL = 3: the f16x3 trunk's (three f16 planes per value, 6 B); PL = 4 (X3Q): the
// hybrid trunk's (two f16 planes and three e4m3 planes per value, 7 B: act_plane / act_q8 below).
template <int NT, int WV, int PL = 0>
struct HeadSmem {
    // 64-candidate tiles (NT = 4) alias pose_encoder.2's output onto pose_encoder.0's (written after
    // a barrier that retires every read of act1), so one workgroup still fits the 160 KiB of a CU
    static constexpr bool kAliasAct = NT >= 4;
    static constexpr int kAct = PL == 4 ? (HID / 32) * NT * 224 : (PL ? (HID / 32) * NT * PL * 64 : KG_HID * NT * 64);   // 16-byte entries
    float xin[NT * 16 * 16];           // input poses, [col][16] (9 used)
    f32x4 act1[kAct];                  // pose_encoder.0 output: [g][ct][lane] (fp32) / [chunk][ct][plane][lane]
    f32x4 act2[kAliasAct ? 4 : kAct];  // pose_encoder.2 output (act1 when aliased)
    // per-wave head-layer-2 partials, wave-minor (head_out reads a row), indexed [v][n][wave] by the
    // value v = (head * NT + column tile) * 3 + output and the column n within the tile: the order the
    // split trunk's reduce-scatter leaves them in (row q of the wave holds values 4g + q); padded to
    // whole groups of four values
    static constexpr int kRedV = (9 * NT + 3) / 4 * 4;
    float red[kRedV][16][WV];
    float xu[NT * 16 * 9];             // PC: last-step mean rows, gathered for the quaternion
    float scratch[WV * 64];
    // small per-launch weights staged once per workgroup (their loads overlap the PC update); the
    // f16x3 trunk holds pose_encoder.0's fragments and bias in registers (SplitScalars)
    f32x4 pe0w[PL ? 1 : 16 * 64];      // pose_encoder.0 packed A fragments
    float pe0b[PL ? 1 : HID], pe2b[HID];
    float h2w[9 * HID];                // head layer 2, [head*3 + out][256]
    float h2b[12];
    f32x4 cscl[NT * 16][2];            // split trunk: per-column scales {s1, s2, u2, uh}, {sh} (ColScales)
};

// Threads [FIRST, WV*64) copy the small weights into LDS. pose_encoder.0's fragments and bias are staged
// for the exact-fp32 trunk only (the split trunk holds them in registers from kernel entry, SplitScalars).
template <int FIRST = 0, int NT, int WV, int PL>
__device__ __forceinline__ void stage_small_weights(const gp_head_weights& w, HeadSmem<NT, WV, PL>& sm) {
    constexpr bool PE0 = PL == 0;
    constexpr int NTH = WV * 64 - FIRST;
    const int t0 = (int)threadIdx.x - FIRST;
    if (t0 < 0) return;
    if constexpr (PE0)
        for (int i = t0; i < 16 * 64; i += NTH) sm.pe0w[i] = ld4(w.pe0_w + (size_t)i * 4);
    for (int i = t0; i < HID; i += NTH) {
        if constexpr (PE0) sm.pe0b[i] = w.pe0_b[i];
        sm.pe2b[i] = w.pe2_b[i];
    }
    for (int i = t0; i < 9 * HID / 4; i += NTH) st4(&sm.h2w[i * 4], ld4(w.h2_w + (size_t)i * 4));
    if (t0 < 9) sm.h2b[t0] = w.h2_b[t0];
}

// Head output o of column c (valid after head_trunk): bias + the per-wave partials in wave order.
// TAN: c is a tangent column of a JVP trunk (below), its output (d head / d pose) . eps has no bias.
template <bool TAN = false, int NT, int WV, int PL>
__device__ __forceinline__ float head_out(const HeadSmem<NT, WV, PL>& sm, int c, int o) {
    const int h = o / 3;
    const int v = (h * NT + (c >> 4)) * 3 + (o - 3 * h);
    float acc = 0.f;
#pragma unroll
    for (int w = 0; w < WV; ++w) acc += sm.red[v][c & 15][w];
    return TAN ? acc : sm.h2b[o] + acc;
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// acc[t][ct] += sum_g A(tile T[t], k-group g) . B(k-group g, column tile ct) over KG k-groups.
// A fragments stream from global (L2-resident packed weights) through a (D+1)-slot register ring
// so that the loads of k-group g+D are in flight while k-group g feeds the MFMAs; B fragments
// come from LDS. Loads are raw buffer loads: the tile/k-group offset is a wave-uniform SGPR
// (soffset) and the only per-lane address is lane*16 (voffset), so the fully unrolled ring needs
// no 64-bit address registers. The k-group loop is unrolled by template recursion, so every ring
// index is a compile-time constant (no scratch).
// Steps G..GEND-1 of the pipelined stream (step G issues k-group G's loads and computes k-group
// G-D). Steps 0..D-1 only prime the ring, so they can be issued early (before a barrier).
template <int G, int GEND, int TT, int NT, int KG, int D>
__device__ __forceinline__ void stream_step(__amdgpu_buffer_rsrc_t W, const int (&T)[TT], const f32x4* __restrict__ B,
                                            int lane, int voff, f32x4 (&ring)[D + 1][TT], f32x4 (&acc)[TT][NT]) {
    if constexpr (G < GEND) {
        if constexpr (G < KG) {
#pragma unroll
            for (int t = 0; t < TT; ++t) ring[G % (D + 1)][t] = ldbuf4(W, voff, (T[t] * KG + G) * 1024);
        }
        // keep the prefetch where it is: without this fence the scheduler sinks every load next to
        // its MFMAs and waits vmcnt(0) per k-group (checked in the .s)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (G >= D) {
            constexpr int GG = G - D;
            f32x4 bf[NT];
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) bf[ct] = B[(GG * NT + ct) * 64 + lane];
            // k-step outermost: consecutive MFMAs hit different accumulators (16x16x4 f32 has a
            // 40-cycle dependent latency vs a 32-cycle issue interval)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < TT; ++t)
#pragma unroll
                    for (int ct = 0; ct < NT; ++ct)
                        acc[t][ct] = mfma4(ring[GG % (D + 1)][t][j], bf[ct][j], acc[t][ct]);
        }
        stream_step<G + 1, GEND, TT, NT, KG, D>(W, T, B, lane, voff, ring, acc);
    }
}

// Forward-mode derivative (JVP) trunks: the upper half of the column tiles (ct >= NT / 2) carries a tangent
// of the lower half's poses (column c + 8 NT is the tangent of column c; its xin row is the direction eps).
// A tangent tile runs through the same GEMMs on the same weight fragments as its primal tile, without the
// bias / pobj / tproj terms, and takes each ReLU's mask from the primal's pre-activation (torch: relu' = 0
// at 0): it sits in the same lane and accumulator slot, so the mask needs no exchange. head_out<true> then
// gives (d head / d pose) . eps.
__device__ __forceinline__ f32x4 mask4(f32x4 d, f32x4 pre) {
    return f32x4{pre.x > 0.f ? d.x : 0.f, pre.y > 0.f ? d.y : 0.f, pre.z > 0.f ? d.z : 0.f, pre.w > 0.f ? d.w : 0.f};
}
// Reverse-pass buffers of the energy-gradient kernels (head_trunk<.., GRAD>, head_backward): cotangents in the
// B-operand layout, [k-group][lane]. g1 (the cotangent of pose_encoder.0's output) takes gh's first 16
// k-groups and the per-wave partials of the pose gradient take g2's: each is written after a barrier that
// retires every read of the buffer it reuses.
struct GradSmem {
    f32x4 gh[3 * KG_HID * 64];   // cotangent of head layer 1's pre-activations, k-group = head * 16 + tile
    f32x4 g2[KG_HID * 64];       // cotangent of pose_encoder.2's pre-activations
};

// Computes the head outputs (read with head_out) for the candidates of this workgroup. Starts with
// the workgroup barrier that publishes sm.xin, obj_of_col and the staged weights (callers write
// them before the call without a barrier of their own; the first weight loads are issued before it).
// `obj_of_col` maps column -> object row of pobj; `tproj` is the 768-vector of this time value.
// GRAD (the energy model's score, grad_x sum_o x_o f_o / sigma): the trunk also leaves the cotangent of head
// layer 1's pre-activations in gs->gh, gh[h][j] = (pre1[h][j] > 0) ? sum_o h2_w[h][o][j] c[3h+o] : 0 with
// c = xin / sigma, formed in the lanes that hold pre1 (the accumulator-native layout is head_backward's B
// operand); act1 and act2 stay live for the reverse pass's masks. The closing barrier is left to
// head_backward, which primes its first weight ring in front of it.
template <int NT, int WV, bool JVP = false, bool GRAD = false>
__device__ __forceinline__ void head_trunk(const gp_head_weights& w, const float* __restrict__ pobj,
                           const float* __restrict__ tproj, const int* obj_of_col, HeadSmem<NT, WV>& sm,
                           int trace_slot = 0, GradSmem* gs = nullptr, float sigma = 1.f) {
    static_assert(!GRAD || (NT == 1 && !JVP), "the reverse pass runs one 16-candidate tile");
    constexpr int TPW = 16 / WV;   // output tiles per wave and per 256-wide layer
    constexpr int NP = JVP ? NT / 2 : NT;   // primal column tiles (tangent tile ct pairs with ct - NP)
    static_assert(!JVP || NT % 2 == 0, "a JVP trunk pairs every primal tile with a tangent tile");
    static_assert(!HeadSmem<NT, WV>::kAliasAct, "the exact-fp32 trunk keeps separate activation buffers");
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform (SGPR)
    const int q = lane >> 4, n = lane & 15;
    const int voff = lane * 16;
    const __amdgpu_buffer_rsrc_t W2 = make_rsrc(w.pe2_w, HID * HID * 4);
    const __amdgpu_buffer_rsrc_t WH = make_rsrc(w.h1p_w, 3 * HID * HID * 4);
    constexpr int D2 = PC_D2, DH = HEAD_PREFETCH;
    int T2[TPW], TH[3 * TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) T2[t] = wid * TPW + t;
#pragma unroll
    for (int h = 0; h < 3; ++h)
#pragma unroll
        for (int t = 0; t < TPW; ++t) TH[h * TPW + t] = h * 16 + wid * TPW + t;
    f32x4 acc2[TPW][NT];
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) acc2[t][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 ring2[D2 + 1][TPW];
    // prime pose_encoder.2's weight ring before pose_encoder.0 (no B operand read yet)
    stream_step<0, D2, TPW, NT, KG_HID, D2>(W2, T2, sm.act1, lane, voff, ring2, acc2);
    __syncthreads();
    PC_MARK(1);
    // ---- pose_encoder.0 (9 -> 256), one k-group
    {
        f32x4 bf[NT];
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) bf[ct] = ld4(&sm.xin[(ct * 16 + n) * 16 + 4 * q]);
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const int T = wid * TPW + t;
            const f32x4 a = sm.pe0w[T * 64 + lane];
            const f32x4 bias = ld4(&sm.pe0b[16 * T + 4 * q]);
            if constexpr (JVP) {
#pragma unroll
                for (int ct = 0; ct < NP; ++ct) {
                    const f32x4 pre = mfma_kgroup(a, bf[ct], f32x4{0.f, 0.f, 0.f, 0.f}) + bias;
                    sm.act1[(T * NT + ct) * 64 + lane] = relu4(pre);
                    sm.act1[(T * NT + NP + ct) * 64 + lane] =
                        mask4(mfma_kgroup(a, bf[NP + ct], f32x4{0.f, 0.f, 0.f, 0.f}), pre);
                }
            } else {
#pragma unroll
                for (int ct = 0; ct < NT; ++ct)
                    sm.act1[(T * NT + ct) * 64 + lane] = relu4(mfma_kgroup(a, bf[ct], f32x4{0.f, 0.f, 0.f, 0.f}) + bias);
            }
        }
    }
    __syncthreads();
    PC_MARK(2);
    // ---- pose_encoder.2 (256 -> 256): TPW output tiles per wave
    // the last PE2_TAIL k-groups of pose_encoder.2 run after the head-layer-1 accumulator-init loads
    // (hoisted pts/t blocks) are issued, so their latency hides behind MFMAs
    constexpr int PE2_TAIL = 4;
    stream_step<D2, KG_HID + D2 - PE2_TAIL, TPW, NT, KG_HID, D2>(W2, T2, sm.act1, lane, voff, ring2, acc2);
    f32x4 tpv[3 * TPW], pov[3 * TPW][NP];
#pragma unroll
    for (int i = 0; i < 3 * TPW; ++i) {
        const int T = TH[i];
        tpv[i] = ld4(tproj + 16 * T + 4 * q);
#pragma unroll
        for (int ct = 0; ct < NP; ++ct) pov[i][ct] = ld4(pobj + (size_t)obj_of_col[ct * 16 + n] * (3 * HID) + 16 * T + 4 * q);
    }
    stream_step<KG_HID + D2 - PE2_TAIL, KG_HID + D2, TPW, NT, KG_HID, D2>(W2, T2, sm.act1, lane, voff, ring2, acc2);
    // ---- head layer 1 prologue, issued before the barrier: the first DH k-groups of the pose-block
    //      weights
    PC_MARK(3);
    f32x4 acc[3 * TPW][NT];
#pragma unroll
    for (int i = 0; i < 3 * TPW; ++i)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            if constexpr (JVP) {
                if (ct < NP) acc[i][ct] = pov[i][ct < NP ? ct : 0] + tpv[i];
                else acc[i][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
                acc[i][ct] = pov[i][ct] + tpv[i];
            }
        }
    f32x4 ringh[DH + 1][3 * TPW];
    stream_step<0, DH, 3 * TPW, NT, KG_HID, DH>(WH, TH, sm.act2, lane, voff, ringh, acc);
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const f32x4 bias = ld4(&sm.pe2b[16 * T2[t] + 4 * q]);
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            if constexpr (JVP)
                sm.act2[(T2[t] * NT + ct) * 64 + lane] =
                    ct < NP ? relu4(acc2[t][ct] + bias) : mask4(acc2[t][ct], acc2[t][ct < NP ? 0 : ct - NP] + bias);
            else
                sm.act2[(T2[t] * NT + ct) * 64 + lane] = relu4(acc2[t][ct] + bias);
        }
    }
    __syncthreads();
    PC_MARK(4);
    // ---- head layer 1 (pose block 256 -> 3x256): 3*TPW output tiles per wave
    stream_step<DH, KG_HID + DH, 3 * TPW, NT, KG_HID, DH>(WH, TH, sm.act2, lane, voff, ringh, acc);
    PC_MARK(5);
    // ---- ReLU -> head layer 2 (block diagonal 3 x (256 -> 3)) partial dot products
#pragma unroll
    for (int h = 0; h < 3; ++h) {
        // GRAD: this lane's column of the cotangent c = x / sigma for head h's three outputs, once per head
        [[maybe_unused]] float c0 = 0.f, c1 = 0.f, c2 = 0.f;
        if constexpr (GRAD) {
            // ld1: three consecutive floats, never merged into one 12-byte LDS read (gp_common.h)
            c0 = fdiv(ld1(&sm.xin[n * 16 + 3 * h + 0]), sigma);
            c1 = fdiv(ld1(&sm.xin[n * 16 + 3 * h + 1]), sigma);
            c2 = fdiv(ld1(&sm.xin[n * 16 + 3 * h + 2]), sigma);
        }
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            float p0 = 0.f, p1 = 0.f, p2 = 0.f;
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                f32x4 u;
                if constexpr (JVP)
                    u = ct < NP ? relu4(acc[h * TPW + t][ct])
                                : mask4(acc[h * TPW + t][ct], acc[h * TPW + t][ct < NP ? 0 : ct - NP]);
                else
                    u = relu4(acc[h * TPW + t][ct]);
                const int ch = 16 * (wid * TPW + t) + 4 * q;
                const f32x4 w0 = ld4(&sm.h2w[(h * 3 + 0) * HID + ch]);
                const f32x4 w1 = ld4(&sm.h2w[(h * 3 + 1) * HID + ch]);
                const f32x4 w2 = ld4(&sm.h2w[(h * 3 + 2) * HID + ch]);
                p0 += u.x * w0.x + u.y * w0.y + u.z * w0.z + u.w * w0.w;
                p1 += u.x * w1.x + u.y * w1.y + u.z * w1.z + u.w * w1.w;
                p2 += u.x * w2.x + u.y * w2.y + u.z * w2.z + u.w * w2.w;
                if constexpr (GRAD)
                    gs->gh[TH[h * TPW + t] * 64 + lane] = mask4(w0 * c0 + w1 * c1 + w2 * c2, acc[h * TPW + t][ct]);
            }
            p0 = rows_sum(p0);
            p1 = rows_sum(p1);
            p2 = rows_sum(p2);
            if (q == 0) {
                sm.red[(h * NT + ct) * 3 + 0][n][wid] = p0;
                sm.red[(h * NT + ct) * 3 + 1][n][wid] = p1;
                sm.red[(h * NT + ct) * 3 + 2][n][wid] = p2;
            }
        }
    }
    if constexpr (!GRAD) __syncthreads();
    PC_MARK(6);
}

#ifndef GRAD_D
#define GRAD_D 4                 // k-groups of transposed weights kept in flight in the reverse pass
#endif

// Reverse pass of head_trunk<1, WV, false, true>: J_f^T c for the 16 candidates, from gs.gh back through head
// layer 1's pose block (h1p_w^T, 256 x 768: 48 k-groups), pose_encoder.2 (pe2_w^T) and pose_encoder.0
// (pe0_w^T, 9 rows padded to one output tile). The transposed weights are packed like the forward ones
// (pack_a_fragments of W^T), so stream_step reads them unchanged, and a layer's output tile T is the next
// layer's k-group T here too. Each ReLU's mask is the forward activation > 0 (act = relu(pre), so the same
// units as pre > 0), in the same lane and slot. Every layer's first GRAD_D k-groups of weights are issued in
// front of the barrier that publishes its B operand. The last layer splits K over the waves (two k-groups
// each); their partial tiles are summed in wave order by pose_grad. Starts with the barrier the GRAD trunk
// leaves out and ends with the one that publishes the partials.
template <int WV>
__device__ __forceinline__ void head_backward(const gp_head_grad_weights& gw, const HeadSmem<1, WV>& sm, GradSmem& gs,
                                              int trace_slot = 0) {
    constexpr int TPW = 16 / WV;
    constexpr int KPW = KG_HID / WV;   // k-groups per wave of the K-split last layer
    constexpr int D = GRAD_D;
    static_assert(KPW * WV == KG_HID && WV * 64 <= KG_HID * 64, "the partial tiles fit g2");
    const int tid = tid_x();
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int voff = lane * 16;
    const __amdgpu_buffer_rsrc_t WH = make_rsrc(gw.h1p_wt, 3 * HID * HID * 4);
    const __amdgpu_buffer_rsrc_t W2 = make_rsrc(gw.pe2_wt, HID * HID * 4);
    const __amdgpu_buffer_rsrc_t W0 = make_rsrc(gw.pe0_wt, 16 * HID * 4);
    int T2[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) T2[t] = wid * TPW + t;
    f32x4 ring[D + 1][TPW];
    f32x4 acc[TPW][1];
    // ---- head layer 1, pose block: g2 = mask(act2) . sum_h W1pose_h^T gh_h
#pragma unroll
    for (int t = 0; t < TPW; ++t) acc[t][0] = f32x4{0.f, 0.f, 0.f, 0.f};
    stream_step<0, D, TPW, 1, 3 * KG_HID, D>(WH, T2, gs.gh, lane, voff, ring, acc);
    __syncthreads();
    PC_MARK(13);
    stream_step<D, 3 * KG_HID + D, TPW, 1, 3 * KG_HID, D>(WH, T2, gs.gh, lane, voff, ring, acc);
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        gs.g2[T2[t] * 64 + lane] = mask4(acc[t][0], sm.act2[T2[t] * 64 + lane]);
        acc[t][0] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // ---- pose_encoder.2: g1 = mask(act1) . pe2_w^T g2 (into gh's first 16 k-groups)
    f32x4* g1 = gs.gh;
    stream_step<0, D, TPW, 1, KG_HID, D>(W2, T2, gs.g2, lane, voff, ring, acc);
    __syncthreads();
    PC_MARK(14);
    stream_step<D, KG_HID + D, TPW, 1, KG_HID, D>(W2, T2, gs.g2, lane, voff, ring, acc);
#pragma unroll
    for (int t = 0; t < TPW; ++t) g1[T2[t] * 64 + lane] = mask4(acc[t][0], sm.act1[T2[t] * 64 + lane]);
    // ---- pose_encoder.0: this wave's k-groups [KPW wid, KPW wid + KPW) of the one output tile, addressed as
    //      "tile wid of a KPW-deep layer"
    const int T0[1] = {wid};
    f32x4 ring0[KPW + 1][1];
    f32x4 acc0[1][1] = {{f32x4{0.f, 0.f, 0.f, 0.f}}};
    stream_step<0, KPW, 1, 1, KPW, KPW>(W0, T0, g1, lane, voff, ring0, acc0);
    __syncthreads();
    PC_MARK(15);
    stream_step<KPW, 2 * KPW, 1, 1, KPW, KPW>(W0, T0, g1 + wid * KPW * 64, lane, voff, ring0, acc0);
    gs.g2[wid * 64 + lane] = acc0[0][0];
    __syncthreads();
}

// (J_f^T c)[o] of column c (valid after head_backward): the waves' partial tiles in wave order. Output row o
// of the tile sits in lane 16 (o / 4) + c, entry o % 4.
template <int WV>
__device__ __forceinline__ float pose_grad(const GradSmem& gs, int c, int o) {
    float acc = 0.f;
#pragma unroll
    for (int w = 0; w < WV; ++w) acc += gs.g2[w * 64 + 16 * (o >> 2) + c][o & 3];
    return acc;
}

// ============================================================================ f16 MFMA helpers
// Split-f16 arithmetic on v_mfma_f32_16x16x32_f16 (16x the fp32 MFMA rate on gfx950). An operand is
// scaled by an exact power of two and split into f16 planes: x = hi + lo (hi = f16(x), lo = f16(x - hi),
// ~22 significant bits; the encoder's SA levels 1-3 and token GEMMs, gp_encoder.hip) or x = hi + mid + lo
// (every bit of an fp32 value: the head trunk below).
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
constexpr int KC_HID = HID / 32;   // 32-deep chunks over a 256-wide activation

__device__ __forceinline__ f32x4 mfma_h(f16x8 a, f16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
// 2^e (e clamped to the normal range) and floor(log2(v)) of a normal v > 0, both exact
__device__ __forceinline__ float exp2i(int e) {
    e = e < -126 ? -126 : (e > 127 ? 127 : e);
    return __uint_as_float((uint32_t)(e + 127) << 23);
}
__device__ __forceinline__ int ilog2f(float v) { return (int)((__float_as_uint(v) >> 23) & 0xff) - 127; }
// max over lanes l, l^16, l^32, l^48
__device__ __forceinline__ float rows_max(float v) {
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
// hi/lo planes of the 32-deep chunk made of two accumulator tiles (u: tile 2c, v: tile 2c+1), times
// s. Lane (q, n) holds k = 4q + j (j < 4) from u and 16 + 4q + j - 4 from v: the k order pack.py's
// pack_h16_fragments gives the weights.
__device__ __forceinline__ void split_pair(f32x4 u, f32x4 v, float s, f16x8& hi, f16x8& lo) {
#pragma clang fp contract(off)
    const float x[8] = {u.x * s, u.y * s, u.z * s, u.w * s, v.x * s, v.y * s, v.z * s, v.w * s};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const _Float16 h = (_Float16)x[j];
        hi[j] = h;
        lo[j] = (_Float16)(x[j] - (float)h);
    }
}

// stream_step on f16 planes over KC 32-deep chunks: ring slot = [tile][hi, lo] of one chunk (2 x 1 KiB
// per tile, weights packed by pack.pack_h16_fragments as [T][chunk][plane][lane]); B = activation
// planes in LDS, [chunk][ct][hi, lo][lane].
template <int KC, int G, int GEND, int TT, int NT, int D>
__device__ __forceinline__ void stream_hk_step(__amdgpu_buffer_rsrc_t W, const int (&T)[TT], const f16x8* __restrict__ B,
                                               int lane, int voff, f16x8 (&ring)[D + 1][TT][2], f32x4 (&acc)[TT][NT]) {
    if constexpr (G < GEND) {
        if constexpr (G < KC) {
#pragma unroll
            for (int t = 0; t < TT; ++t)
#pragma unroll
                for (int p = 0; p < 2; ++p)
                    ring[G % (D + 1)][t][p] =
                        __builtin_bit_cast(f16x8, ldbuf4(W, voff, ((T[t] * KC + G) * 2 + p) * 1024));
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (G >= D && NT > 4) {
            // wide column blocks (encoder levels 2-3): one column tile's planes live at a time
            constexpr int GG = G - D, S = GG % (D + 1);
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                const f16x8 bh = B[((GG * NT + ct) * 2 + 0) * 64 + lane];
                const f16x8 bl = B[((GG * NT + ct) * 2 + 1) * 64 + lane];
#pragma unroll
                for (int t = 0; t < TT; ++t) acc[t][ct] = mfma_h(ring[S][t][1], bh, acc[t][ct]);
#pragma unroll
                for (int t = 0; t < TT; ++t) acc[t][ct] = mfma_h(ring[S][t][0], bl, acc[t][ct]);
#pragma unroll
                for (int t = 0; t < TT; ++t) acc[t][ct] = mfma_h(ring[S][t][0], bh, acc[t][ct]);
            }
        } else if constexpr (G >= D) {
            constexpr int GG = G - D, S = GG % (D + 1);
            f16x8 bh[NT], bl[NT];
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                bh[ct] = B[((GG * NT + ct) * 2 + 0) * 64 + lane];
                bl[ct] = B[((GG * NT + ct) * 2 + 1) * 64 + lane];
            }
#pragma unroll
            for (int t = 0; t < TT; ++t)
#pragma unroll
                for (int ct = 0; ct < NT; ++ct) acc[t][ct] = mfma_h(ring[S][t][1], bh[ct], acc[t][ct]);
#pragma unroll
            for (int t = 0; t < TT; ++t)
#pragma unroll
                for (int ct = 0; ct < NT; ++ct) acc[t][ct] = mfma_h(ring[S][t][0], bl[ct], acc[t][ct]);
#pragma unroll
            for (int t = 0; t < TT; ++t)
#pragma unroll
                for (int ct = 0; ct < NT; ++ct) acc[t][ct] = mfma_h(ring[S][t][0], bh[ct], acc[t][ct]);
        }
        stream_hk_step<KC, G + 1, GEND, TT, NT, D>(W, T, B, lane, voff, ring, acc);
    }
}


// The split trunk's activation bounds and weight exponents (gp_head_weights.hsc). Loaded at kernel entry by
// the callers: read where they are used, their round trip (a cold L2 line after the kernel boundary) sat
// on the critical path between the PC update and pose_encoder.0.
// Also this wave's pose_encoder.0 A fragments and bias (output tiles 2 wid, 2 wid + 1 of an 8-wave
// workgroup): loaded at kernel entry instead of being staged through LDS for every launch.
constexpr int HSPLIT_WV = 8;   // waves per workgroup of the split-trunk kernels
struct SplitScalars {
    float A0, B0, A2, B2;
    int ew2, ewh;
    f32x4 pe0a[4], pe0b[4];   // this wave's 16 / WV output tiles (entries past them unused)
};
// PL = 0 (the exact-fp32 trunk, which has none): zeros, nothing loaded.
template <int PL, int WV = HSPLIT_WV>
__device__ __forceinline__ SplitScalars load_split_scalars(const gp_head_weights& w) {
    static_assert(WV == 4 || WV == 8, "the split trunk runs 4- or 8-wave workgroups");
    if constexpr (PL == 0) {
        return SplitScalars{};
    } else {
        const f32x4 a = ld4(w.hsc), b = ld4(w.hsc + 4);
        SplitScalars r{a.x, a.y, a.z, a.w, (int)b.x, (int)b.y, {}, {}};
        const int tid = tid_x();
        const int lane = tid & 63, q = lane >> 4;
        const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
        for (int t = 0; t < 16 / WV; ++t) {
            const int T = wid * (16 / WV) + t;
            r.pe0a[t] = ld4(w.pe0_w + ((size_t)T * 64 + lane) * 4);
            r.pe0b[t] = ld4(w.pe0_b + 16 * T + 4 * q);
        }
        return r;
    }
}

// Sums of four values over the four 16-lane rows, scattered: on return row q of the wave holds the
// total of value q (its column n's sum over lanes n, n+16, n+32, n+48). Three row swaps and three adds
// for four values (a full row sum of each would take eight and eight); the pairs are summed in
// rows_sum's order, (r0 + r1) + (r2 + r3), so each total has rows_sum's bits.
// v_permlane16_swap exchanges the odd rows of its first operand with the even rows of its second;
// v_permlane32_swap the upper half of the first with the lower half of the second.
__device__ __forceinline__ float rows_sum_scatter4(float a, float b, float c, float d) {
    const auto ab = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    const auto cd = __builtin_amdgcn_permlane16_swap(__float_as_uint(c), __float_as_uint(d), false, false);
    const float s = __uint_as_float(ab[0]) + __uint_as_float(ab[1]);   // rows: a01, b01, a23, b23
    const float t = __uint_as_float(cd[0]) + __uint_as_float(cd[1]);   // rows: c01, d01, c23, d23
    const auto st = __builtin_amdgcn_permlane32_swap(__float_as_uint(s), __float_as_uint(t), false, false);
    return __uint_as_float(st[0]) + __uint_as_float(st[1]);            // rows: a, b, c, d
}

// A candidate's power-of-two scales of the split trunk from m0 = max |pose entry| (rigorous bounds of
// pose_encoder.0's and .2's outputs, hs): s1 / s2 scale the two activations into [2^14, 2^15) at their
// bound, u2 / uh undo both scales of pose_encoder.2 / head layer 1, sh brings head layer 1's fp32 init
// into the scaled domain. One definition for the trunk and the PC update waves that precompute it.
struct ColScales {
    float s1, s2, u2, uh, sh;
};
__device__ __forceinline__ ColScales split_col_scales(float m0, const SplitScalars& hs) {
    const float b1 = fmaxf(__builtin_fmaf(hs.A0, m0, hs.B0) * 1.0009765625f, 1e-18f);
    const float b2 = fmaxf(__builtin_fmaf(hs.A2, b1, hs.B2) * 1.0009765625f, 1e-18f);
    const int e1 = ilog2f(b1), e2 = ilog2f(b2);
    return ColScales{exp2i(14 - e1), exp2i(14 - e2), exp2i(e1 - 14 - hs.ew2), exp2i(e2 - 14 - hs.ewh),
                     exp2i(14 - e2 + hs.ewh)};
}
// max |x| of a 16-wide xin row held four entries per lane over the four 16-lane rows (the trunk's
// B-operand layout): the bound's m0
__device__ __forceinline__ float xin_row_absmax(f32x4 b) {
    return rows_max(fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fmaxf(fabsf(b.z), fabsf(b.w))));
}

// ============================================================================ f16x3 trunk
// The two per-candidate GEMMs (pose_encoder.2 and head layer 1's pose block) on
// v_mfma_f32_16x16x32_f16 with three f16 planes per operand: after an exact power-of-two scaling,
// x = hi + mid + lo with hi = f16(x), mid = f16(x - hi), lo = f16(x - hi - mid) holds every bit of an
// fp32 value (11 + 11 + 11 >= 24 significant bits; only values ~2^-7 below the operand's scale lose
// lo bits to f16 subnormals, an absolute error <= 2^-39 of the scale). Per 32-deep chunk, the six
// products whose plane orders sum to <= 2 (relative sizes 1, 2^-11, 2^-11, 2^-22 x3) are formed; the
// three dropped ones are <= 2^-33 relative, so every product w*a enters the sum to ~2^-33, finer than
// an fp32 FMA. hi*hi accumulates in one fp32 accumulator (one rounding per 32-deep chunk, as the
// MFMA sums its 32 exact f16 products and rounds once), the five cross products in a second one (its
// roundings are 2^-11 smaller), and the two are added once per layer: fewer roundings at full
// magnitude than v_mfma_f32_16x16x4_f32's one per 4-deep step (scripts/precision_study3.py,
// scripts/mfma_round_probe.hip). Six f16 MFMAs per 32x16x16 chunk-tile take 96 cycles against the
// exact fp32 MFMA's 256.
// Weights: per-layer exponents and packed hi/mid/lo planes (pack.pack_h16_fragments, 6 B per weight).
// Activations: a per-candidate exponent from a rigorous bound on the layer's outputs (max|pose| times
// the layer's max row L1 norm plus max|bias|, chained), so no extra barrier is needed and f16 cannot
// overflow. pose_encoder.0 and head layer 2 stay fp32 (VALU / fp32 MFMA).
#ifndef X3_D2
#define X3_D2 2                  // 32-deep chunks of pose_encoder.2 weights kept in flight
#endif
#ifndef X3_DH
#define X3_DH 1                  // 32-deep chunks of head-layer-1 weights kept in flight (2: ab_prio_dh1.json)
#endif
constexpr int X3P = 3;           // planes per operand

// ---- hybrid form (PL = X3Q): the three products of plane order 2 on block-scaled FP8 MFMA
// Of the six products, hi*hi, hi*mid and mid*hi carry everything down to 2^-22 of the leading product and stay
// on f16; w_hi*a_lo, w_mid*a_mid and w_lo*a_hi are each <= 2^-22 of it, so e4m3's four significant bits per
// operand leave their error near 2^-26 per product (scripts/x3q_error_model.py: the score error stays below
// exact fp32's). They run on v_mfma_scale_f32_16x16x128_f8f6f4, one instruction per product and 128-deep group
// (32 cycles against the 4 x 16 of the f16 form), into `cor`: per 128-deep group and tile 12 f16 + 3 FP8
// MFMAs, 288 cycles against 384.
// An e4m3 plane is the f16 plane times a constant power of two that brings the plane's bound to 2^7..2^8
// (hi < 2^15 -> x 2^-7, |mid| <= 2^3 -> x 2^4, |lo| <= 2^-9 -> x 2^16; e4m3's largest value is 448), converted
// with v_cvt_scalef32_pk_fp8_f16 (q8_of: round to nearest even, subnormals kept). The MFMA's E8M0 block scales,
// constants, undo the two planes' constants, so the products enter `cor` in the scaled domain of the f16 ones.
// Product k of a group is issued with chunk 4g + k of the f16 stream (k < 3), its A planes riding in that chunk's
// ring slot. Lane (q, i) of an operand holds 32 bytes per group: byte 8 cc + j is element j of the lane's f16
// fragment of chunk 4g + cc (the same k in A and B, which is all the sum needs).
// LDS, per activation buffer (16-byte entries): f16 planes [chunk][ct][hi, mid][lane], then the e4m3 planes
// [group][ct][product][half][lane] (product k's B operand: a_lo8, a_mid8, a_hi8).
// Weights: pack.pack_q8_fragments, [T][group][product][half][lane] (w_hi8, w_mid8, w_lo8).
constexpr int X3Q = 4;           // HeadSmem / trunk PL of the hybrid form
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
constexpr int Q8_EXP_HI = -7, Q8_EXP_MID = 4, Q8_EXP_LO = 16;   // e4m3 plane = f16 plane x 2^this
template <int PL>
constexpr int act_f16_planes() { return PL == X3Q ? 2 : X3P; }
// 16-byte entry of f16 plane p of (chunk, column tile), lane 0
template <int PL, int NT>
__device__ __forceinline__ constexpr int act_plane(int chunk, int ct, int p) {
    return ((chunk * NT + ct) * act_f16_planes<PL>() + p) * 64;
}
// 16-byte entry of half h of product k's e4m3 B operand of (group, column tile), lane 0
template <int NT>
__device__ __forceinline__ constexpr int act_q8(int group, int ct, int k, int h) {
    return KC_HID * NT * 2 * 64 + (((group * NT + ct) * 3 + k) * 2 + h) * 64;
}
// product k of w (A) and activation (B) e4m3 planes, c += A . B x 2^-(the two planes' exponents)
template <int K>
__device__ __forceinline__ f32x4 mfma_q8(f16x8 a0, f16x8 a1, f16x8 b0, f16x8 b1, f32x4 c) {
    using u4 = __attribute__((ext_vector_type(4))) int;
    const u4 x0 = __builtin_bit_cast(u4, a0), x1 = __builtin_bit_cast(u4, a1);
    const u4 y0 = __builtin_bit_cast(u4, b0), y1 = __builtin_bit_cast(u4, b1);
    const i32x8 a = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
    const i32x8 b = {y0[0], y0[1], y0[2], y0[3], y1[0], y1[1], y1[2], y1[3]};
    // weight planes hi8, mid8, lo8 meet activation planes lo8, mid8, hi8
    constexpr int ea = K == 0 ? Q8_EXP_HI : (K == 1 ? Q8_EXP_MID : Q8_EXP_LO);
    constexpr int eb = K == 0 ? Q8_EXP_LO : (K == 1 ? Q8_EXP_MID : Q8_EXP_HI);
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 127 - ea, 0, 127 - eb);
}
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));
// The 8 e4m3 bytes of one f16 fragment times 2^E (element j -> byte j), converted from the packed f16 pairs under
// the scale in one v_cvt_scalef32_pk_fp8_f16 per pair: the instruction divides by its scale operand (2^-E here),
// rounds to nearest even and keeps e4m3 subnormals and f16 subnormal inputs, so on finite |p 2^E| <= 256 its bytes
// are those of v_cvt_pk_fp8_f32((float)p * 2^E) (every f16 pattern x the three planes: gp_debug_q8_probe,
// tests/test_gpu_plane_epilogue.py). VIA_F32: that earlier path (two conversions back, two multiplications and
// one conversion per pair), kept for the probe's comparison only.
template <int E, bool VIA_F32 = false>
__device__ __forceinline__ u32x2 q8_of(f16x8 p) {
    if constexpr (VIA_F32) {
        const float s = exp2i(E);
        int lo = 0, hi = 0;
        lo = __builtin_amdgcn_cvt_pk_fp8_f32((float)p[0] * s, (float)p[1] * s, lo, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32((float)p[2] * s, (float)p[3] * s, lo, true);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32((float)p[4] * s, (float)p[5] * s, hi, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32((float)p[6] * s, (float)p[7] * s, hi, true);
        return u32x2{(unsigned)lo, (unsigned)hi};
    } else {
        const float s = exp2i(-E);
        // each conversion replaces one 16-bit word of its destination and the two of a register replace both: the
        // destination starts undefined instead of costing a v_mov 0 (an empty asm defines it; its input only keeps
        // the two asms of a fragment, and those of other fragments, from being merged into one value)
        i16x2 lo, hi;
        asm("" : "=v"(lo) : "v"(f16x2{p[0], p[1]}));
        asm("" : "=v"(hi) : "v"(f16x2{p[4], p[5]}));
        lo = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(lo, f16x2{p[0], p[1]}, s, false);
        lo = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(lo, f16x2{p[2], p[3]}, s, true);
        hi = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(hi, f16x2{p[4], p[5]}, s, false);
        hi = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(hi, f16x2{p[6], p[7]}, s, true);
        return u32x2{__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi)};
    }
}
// One (chunk, column tile)'s planes as the epilogues hold them between the split and the LDS write
template <int PL>
struct ActPlanes {
    f16x8 h[act_f16_planes<PL>()];
    u32x2 q[PL == X3Q ? 3 : 1];   // X3Q: the e4m3 bytes of products 0..2's B operands (a_lo8, a_mid8, a_hi8)
};

// x - (float)h for half HI of the packed pair h, in one v_fma_mix_f32 that reads the f16 operand in place:
// h * -1 + x, an exact product under the subtraction's single rounding, so the bits (and the sign of a zero) are
// those of converting h back and subtracting. Written as asm: from C the compiler turns fma(h, -1, x) back into
// v_cvt_f32_f16 + v_sub_f32.
template <int HI>
__device__ __forceinline__ float sub_f16(float x, f16x2 h) {
    float r;
    if constexpr (HI)
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(x));
    else
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(x));
    return r;
}
// {f16(x[0] - h[0]), f16(x[1] - h[1])}: the same residuals converted to f16 by the instruction that forms them
// (v_fma_mixlo_f16 / v_fma_mixhi_f16: the residual is exact in fp32, so the conversion is the only rounding)
__device__ __forceinline__ f16x2 sub_f16_pk(f32x2 x, f16x2 h) {
    f16x2 d;
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(h), "v"(x[0]));
    asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(d) : "v"(h), "v"(x[1]));
    return d;
}
// The three planes of the 32-deep chunk made of two accumulator tiles (u: tile 2c, v: tile 2c+1),
// times s, in the k order of pack_h16_fragments (as split_pair): x = h + m + l exactly (x finite, |x| < 65504;
// f16 subnormals aside) with h = f16(x), m = f16(x - h), l = f16(x - h - m). Both residuals are exact (x and h
// agree in sign and leading bits; <= 3 significant bits remain for l). Two values at a time, each plane's pair
// packed by the conversion that makes it.
__device__ __forceinline__ void split3_pair(f32x4 u, f32x4 v, float s, f16x8 (&p)[X3P]) {
#pragma clang fp contract(off)
    const float x[8] = {u.x * s, u.y * s, u.z * s, u.w * s, v.x * s, v.y * s, v.z * s, v.w * s};
    f16x2 h[4], m[4], l[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        h[j] = __builtin_convertvector(f32x2{x[2 * j], x[2 * j + 1]}, f16x2);
        const f32x2 r = {sub_f16<0>(x[2 * j], h[j]), sub_f16<1>(x[2 * j + 1], h[j])};
        m[j] = __builtin_convertvector(r, f16x2);
        l[j] = sub_f16_pk(r, m[j]);
    }
    p[0] = __builtin_shufflevector(__builtin_shufflevector(h[0], h[1], 0, 1, 2, 3),
                                   __builtin_shufflevector(h[2], h[3], 0, 1, 2, 3), 0, 1, 2, 3, 4, 5, 6, 7);
    p[1] = __builtin_shufflevector(__builtin_shufflevector(m[0], m[1], 0, 1, 2, 3),
                                   __builtin_shufflevector(m[2], m[3], 0, 1, 2, 3), 0, 1, 2, 3, 4, 5, 6, 7);
    p[2] = __builtin_shufflevector(__builtin_shufflevector(l[0], l[1], 0, 1, 2, 3),
                                   __builtin_shufflevector(l[2], l[3], 0, 1, 2, 3), 0, 1, 2, 3, 4, 5, 6, 7);
}
// split3_pair into the planes the PL form keeps: X3P the three f16 planes; X3Q hi, mid and the e4m3 planes
template <int PL>
__device__ __forceinline__ void split_act(f32x4 u, f32x4 v, float s, ActPlanes<PL>& a) {
    f16x8 p[X3P];
    split3_pair(u, v, s, p);
    a.h[0] = p[0];
    a.h[1] = p[1];
    if constexpr (PL == X3Q) {
        a.q[0] = q8_of<Q8_EXP_LO>(p[2]);
        a.q[1] = q8_of<Q8_EXP_MID>(p[1]);
        a.q[2] = q8_of<Q8_EXP_HI>(p[0]);
    } else {
        a.h[2] = p[2];
    }
}
// ... written to the activation buffer `act` as (chunk, column tile ct)'s B planes
template <int PL, int NT>
__device__ __forceinline__ void store_act(f16x8* act, int chunk, int ct, int lane, const ActPlanes<PL>& a) {
#pragma unroll
    for (int p = 0; p < act_f16_planes<PL>(); ++p) act[act_plane<PL, NT>(chunk, ct, p) + lane] = a.h[p];
    if constexpr (PL == X3Q) {
        const int cc = chunk & 3;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            reinterpret_cast<u32x2*>(act + act_q8<NT>(chunk >> 2, ct, k, cc >> 1) + lane)[cc & 1] = a.q[k];
    }
}
// One pipelined step of a 256-deep f16x3 layer: step G issues the loads of chunk G (tile T[t]'s three
// weight planes, 3 KiB per tile: pack_h16_fragments' [T][c][plane][lane]) and computes chunk G - D from
// the ring; B = activation planes in LDS, [chunk][ct][plane][lane]. acc += hi*hi, cor += the five cross
// products, smallest first. The B planes of column tile ct + 1 are read while column tile ct's MFMAs
// run (sched barriers keep the compiler from sinking the reads to their first use, where
// each became an lgkmcnt(0) stall). Steps 0..D-1 only prime the ring (no B or accumulator access), so
// they can run before a barrier or under another phase.
// PL = X3Q (hybrid): a ring slot holds the chunk's hi and mid planes and, for a chunk that carries a product
// (G % 4 < 3), the two halves of that product's e4m3 A operand from WQ; cor += product k, mid*hi, hi*mid.
template <int PL>
constexpr int ring_planes() { return PL == X3Q ? 4 : X3P; }
// The B planes of (chunk GG, column tile ct): the f16 planes, then (X3Q, a chunk with a product) its e4m3 halves
template <int PL, int NT>
__device__ __forceinline__ void load_b_planes(const f16x8* __restrict__ B, int GG, int ct, int lane,
                                              f16x8 (&b)[ring_planes<PL>()]) {
#pragma unroll
    for (int p = 0; p < act_f16_planes<PL>(); ++p) b[p] = B[act_plane<PL, NT>(GG, ct, p) + lane];
    if constexpr (PL == X3Q) {
        if ((GG & 3) < 3) {
            b[2] = B[act_q8<NT>(GG >> 2, ct, GG & 3, 0) + lane];
            b[3] = B[act_q8<NT>(GG >> 2, ct, GG & 3, 1) + lane];
        }
    }
}
// One tile's correction products of chunk GG (KQ = GG % 4): X3P smallest first; X3Q the 8-pass FP8 instruction
// last, so that the MFMA issued after it (another tile's or the main product) does not wait for its result
template <int PL, int KQ>
__device__ __forceinline__ f32x4 cross_products(const f16x8 (&w)[ring_planes<PL>()], const f16x8 (&b)[ring_planes<PL>()],
                                                f32x4 c) {
    if constexpr (PL != X3Q) {
        c = mfma_h(w[2], b[0], c);
        c = mfma_h(w[0], b[2], c);
        c = mfma_h(w[1], b[1], c);
    }
    c = mfma_h(w[1], b[0], c);
    c = mfma_h(w[0], b[1], c);
    if constexpr (PL == X3Q && KQ < 3) c = mfma_q8<KQ < 3 ? KQ : 0>(w[2], w[3], b[2], b[3], c);
    return c;
}
template <int PL, int G, int GEND, int TT, int NT, int D>
__device__ __forceinline__ void stream_x3_rec(__amdgpu_buffer_rsrc_t W, __amdgpu_buffer_rsrc_t WQ, const int (&T)[TT],
                                              const f16x8* __restrict__ B, int lane, int voff,
                                              f16x8 (&ring)[D + 1][TT][ring_planes<PL>()], f32x4 (&acc)[TT][NT],
                                              f32x4 (&cor)[TT][NT], f16x8 (&bc)[ring_planes<PL>()]) {
    constexpr int RP = ring_planes<PL>();
    if constexpr (G < GEND) {
        if constexpr (G < KC_HID) {
#pragma unroll
            for (int t = 0; t < TT; ++t) {
#pragma unroll
                for (int p = 0; p < act_f16_planes<PL>(); ++p)
                    ring[G % (D + 1)][t][p] =
                        __builtin_bit_cast(f16x8, ldbuf4(W, voff, ((T[t] * KC_HID + G) * X3P + p) * 1024));
                if constexpr (PL == X3Q && (G & 3) < 3) {
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        ring[G % (D + 1)][t][2 + h] = __builtin_bit_cast(
                            f16x8, ldbuf4(WQ, voff, (((T[t] * (KC_HID / 4) + G / 4) * 3 + (G & 3)) * 2 + h) * 1024));
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (G >= D) {
            constexpr int GG = G - D, S = GG % (D + 1), KQ = GG & 3;
            // B planes one column tile ahead: column tile ct + 1's (or the next chunk's first) reads are in
            // flight during column tile ct's MFMAs (just-in-time reads: profiles/r4/ab_bpipe.json)
            if constexpr (GG == 0) load_b_planes<PL, NT>(B, 0, 0, lane, bc);
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                f16x8 bn[RP];
                const int ng = ct + 1 < NT ? GG : GG + 1, nc = ct + 1 < NT ? ct + 1 : 0;
                if (ct + 1 < NT || GG + 1 < KC_HID) load_b_planes<PL, NT>(B, ng, nc, lane, bn);
                __builtin_amdgcn_sched_barrier(0);   // the reads stay ahead of this column tile's MFMAs
                f16x8 b[RP];
#pragma unroll
                for (int p = 0; p < RP; ++p) b[p] = bc[p];
                // each tile's correction products back to back on one accumulator, then the main
                // products (the issue rate itself does not depend on the order, scripts/mfma_chain_probe.hip;
                // this order measured 3 % faster at R=25,600 (two passes), even at R=12,800 (one):
                // profiles/r4/ab_chain.json)
#pragma unroll
                for (int t = 0; t < TT; ++t) {
                    cor[t][ct] = cross_products<PL, KQ>(ring[S][t], b, cor[t][ct]);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int t = 0; t < TT; ++t) acc[t][ct] = mfma_h(ring[S][t][0], b[0], acc[t][ct]);
                __builtin_amdgcn_sched_barrier(0);
                if (ct + 1 < NT || GG + 1 < KC_HID) {
#pragma unroll
                    for (int p = 0; p < RP; ++p) bc[p] = bn[p];
                }
            }
        }
        stream_x3_rec<PL, G + 1, GEND, TT, NT, D>(W, WQ, T, B, lane, voff, ring, acc, cor, bc);
    }
}
// The weight planes a trunk streams: the f16 planes and, for the hybrid form, the e4m3 ones (W again otherwise)
struct X3Weights {
    __amdgpu_buffer_rsrc_t W, WQ;
};
template <int PL, int G, int GEND, int TT, int NT, int D>
__device__ __forceinline__ void stream_x3_step(const X3Weights& w, const int (&T)[TT], const f16x8* __restrict__ B,
                                               int lane, int voff, f16x8 (&ring)[D + 1][TT][ring_planes<PL>()],
                                               f32x4 (&acc)[TT][NT], f32x4 (&cor)[TT][NT]) {
    f16x8 bc[ring_planes<PL>()];   // the B planes of the next column tile, carried from step to step
    stream_x3_rec<PL, G, GEND, TT, NT, D>(w.W, w.WQ, T, B, lane, voff, ring, acc, cor, bc);
}

// The fp32 init rows of head layer 1 (hoisted pts + t blocks: pobj of each column's object, tproj) for this
// wave's output tiles of head H: loads issued where their latency hides (under the previous head's epilogue,
// or the pose_encoder.2 epilogue for head 0) and folded into the accumulator at the head's start, so they are
// not live across the MFMA stream.
template <int H, int NT, int TPW, int NP = NT>   // NP: column tiles with init rows (the primal tiles of a JVP trunk)
__device__ __forceinline__ void head_x3_init_load(__amdgpu_buffer_rsrc_t RP, __amdgpu_buffer_rsrc_t RT, const int (&vo)[NT],
                                                  int wid, int lane, f32x4 (&tpv)[TPW], f32x4 (&pov)[TPW][NP]) {
    const int q = lane >> 4;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int T = H * 16 + wid * TPW + t;
        tpv[t] = ldbuf4(RT, 16 * q, 64 * T);
#pragma unroll
        for (int ct = 0; ct < NP; ++ct) pov[t][ct] = ldbuf4(RP, vo[ct], 64 * T);
    }
}

// head_trunk with the f16x3 GEMMs (same contract: head_out reads the outputs after it returns).
// Head layer 1 runs one head at a time (2 output tiles per wave and head): the head's fp32 init rows
// enter its main accumulator in the scaled domain (x sh, a power of two: exact), hi*hi accumulates on top
// and the cross products beside it; the next head's first weight chunks and init rows are in flight during
// this head's layer-2 partials.
// PRE: the caller wrote every column's ColScales to sm.cscl before the trunk's first barrier (the PC
// step's update waves, which hold the rows), so the trunk reads them instead of recomputing them in
// every wave.
template <int H, int NT, int WV, int TPW, int DH, bool JVP = false, int PL = X3P>
__device__ __forceinline__ void head_x3_head(const X3Weights& WH, const f16x8* __restrict__ act2h,
                                             __amdgpu_buffer_rsrc_t RP, __amdgpu_buffer_rsrc_t RT, const int (&vo)[NT],
                                             HeadSmem<NT, WV, PL>& sm, const float (&uh)[NT], const float (&sh)[NT],
                                             int wid, int lane, f16x8 (&ringh)[DH + 1][TPW][ring_planes<PL>()],
                                             f32x4 (&tpv)[TPW], f32x4 (&pov)[TPW][JVP ? NT / 2 : NT],
                                             float (&pv)[HeadSmem<NT, WV, PL>::kRedV]) {
    constexpr int NP = JVP ? NT / 2 : NT;
    const int q = lane >> 4, n = lane & 15;
    const int voff = lane * 16;
    int TH[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) TH[t] = H * 16 + wid * TPW + t;
    f32x4 acc[TPW][NT], cor[TPW][NT];
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            if (ct < NP) acc[t][ct] = (pov[t][ct] + tpv[t]) * sh[ct];
            else acc[t][ct] = f32x4{0.f, 0.f, 0.f, 0.f};   // a tangent tile has no init rows
            cor[t][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    stream_x3_step<PL, DH, KC_HID + DH, TPW, NT, DH>(WH, TH, act2h, lane, voff, ringh, acc, cor);
    if constexpr (H < 2) {   // the next head's first chunks and init rows, in flight across this epilogue
        int TN[TPW];
#pragma unroll
        for (int t = 0; t < TPW; ++t) TN[t] = TH[t] + 16;
        stream_x3_step<PL, 0, DH, TPW, NT, DH>(WH, TN, act2h, lane, voff, ringh, acc, cor);
        head_x3_init_load<H + 1, NT, TPW, NP>(RP, RT, vo, wid, lane, tpv, pov);
    }
    // nothing below is scheduled into the MFMA stream above: interleaved there, the row swaps of the
    // reduce-scatter reused registers in-flight MFMAs still read (v_permlane*_swap writes both operands)
    __builtin_amdgcn_sched_barrier(0);
    // ReLU -> head layer 2 (block diagonal 3 x (256 -> 3)) partials of this head's accumulators (scaled domain;
    // uh[ct], a power of two, undoes the scale exactly). Each (column, output) is one fp32 FMA chain over this
    // wave's channels, t-major then j, with separately rounded sums across rows and waves (head_out).
    float p[NT][3];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) p[ct][0] = p[ct][1] = p[ct][2] = 0.f;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int ch = 16 * (wid * TPW + t) + 4 * q;
        const f32x4 w0 = ld4(&sm.h2w[(H * 3 + 0) * HID + ch]);
        const f32x4 w1 = ld4(&sm.h2w[(H * 3 + 1) * HID + ch]);
        const f32x4 w2 = ld4(&sm.h2w[(H * 3 + 2) * HID + ch]);
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            f32x4 u;
            if constexpr (JVP) {
                constexpr int NPP = JVP ? NP : 0;
                const int cp = ct < NPP ? 0 : ct - NPP;   // a tangent tile's primal tile
                u = ct < NPP ? relu4((acc[t][ct] + cor[t][ct]) * uh[ct])
                             : mask4((acc[t][ct] + cor[t][ct]) * uh[ct], (acc[t][cp] + cor[t][cp]) * uh[cp]);
            } else {
                u = relu4((acc[t][ct] + cor[t][ct]) * uh[ct]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                p[ct][0] = __builtin_fmaf(u[j], w0[j], p[ct][0]);
                p[ct][1] = __builtin_fmaf(u[j], w1[j], p[ct][1]);
                p[ct][2] = __builtin_fmaf(u[j], w2[j], p[ct][2]);
            }
        }
    }
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
        for (int o = 0; o < 3; ++o) pv[(H * NT + ct) * 3 + o] = p[ct][o];
    // rows reduce-scatter (rows_sum_scatter4) of this head's values where they fill whole groups of four
    if constexpr ((3 * NT) % 4 == 0) {
#pragma unroll
        for (int g = H * 3 * NT / 4; g < (H + 1) * 3 * NT / 4; ++g)
            sm.red[4 * g + q][n][wid] = rows_sum_scatter4(pv[4 * g], pv[4 * g + 1], pv[4 * g + 2], pv[4 * g + 3]);
    }
    __builtin_amdgcn_sched_barrier(0);
}

// Entry i of column c's precomputed ColScales in sm.cscl (0 s1, 1 s2, 2 u2, 3 uh, 4 sh), one 4-byte read (ld1: parts
// of a row read at different places are not merged into a 12-byte read)
template <int NT, int WV, int PL>
__device__ __forceinline__ float col_scale(const HeadSmem<NT, WV, PL>& sm, int c, int i) {
    return ld1(reinterpret_cast<const float*>(&sm.cscl[c][0]) + i);
}

// PL (taken from sm): X3P the six f16 products; X3Q the hybrid form (w.pe2_q / w.h1p_q must be given)
template <int NT, int WV, bool PRE = false, bool JVP = false, int PL = X3P>
__device__ __forceinline__ void head_trunk_x3(const gp_head_weights& w, const float* __restrict__ pobj,
                                              const float* __restrict__ tproj, const int* obj_of_col,
                                              HeadSmem<NT, WV, PL>& sm, int trace_slot, const SplitScalars hs) {
    static_assert(PL == X3P || (PL == X3Q && !JVP), "the hybrid form has no tangent tiles");
    constexpr int TPW = 16 / WV;   // output tiles per wave and 256-wide layer; tiles (2c, 2c+1) form chunk c
    static_assert(TPW % 2 == 0, "the f16x3 trunk pairs a wave's output tiles into 32-deep chunks");
    static_assert(TPW <= 4, "SplitScalars carries at most four pose_encoder.0 tiles per wave");
    constexpr int CPW = TPW / 2;
    constexpr int NP = JVP ? NT / 2 : NT;   // primal column tiles (tangent tile ct pairs with ct - NP)
    static_assert(!JVP || NT % 2 == 0, "a JVP trunk pairs every primal tile with a tangent tile");
    using SM = HeadSmem<NT, WV, PL>;
    const int tid = tid_x();
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane >> 4, n = lane & 15;
    const int voff = lane * 16;
    X3Weights W2, WH;
    W2.W = W2.WQ = make_rsrc(w.pe2_h, HID * HID * 2 * X3P);
    WH.W = WH.WQ = make_rsrc(w.h1p_h, 3 * HID * HID * 2 * X3P);
    if constexpr (PL == X3Q) {
        W2.WQ = make_rsrc(w.pe2_q, HID * HID * 3);
        WH.WQ = make_rsrc(w.h1p_q, 3 * HID * HID * 3);
    }
    f16x8* act1h = reinterpret_cast<f16x8*>(sm.act1);
    f16x8* act2h = reinterpret_cast<f16x8*>(SM::kAliasAct ? sm.act1 : sm.act2);
    constexpr int D2 = X3_D2, DH = X3_DH;
    int T2[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) T2[t] = wid * TPW + t;
    f32x4 acc2[TPW][NT], cor2[TPW][NT];
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) acc2[t][ct] = cor2[t][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    f16x8 ring2[D2 + 1][TPW][ring_planes<PL>()];
    stream_x3_step<PL, 0, D2, TPW, NT, D2>(W2, T2, act1h, lane, voff, ring2, acc2, cor2);
    __syncthreads();
    PC_MARK(1);
    // ---- per-candidate exponents: bound1 >= |pose_encoder.0 out|, bound2 >= |pose_encoder.2 out|
    // LATE_SCALES (the 64-candidate hybrid PC step, which sits at the 256-register limit): the later layers' scales
    // are read from sm.cscl where they are used (ahead of pose_encoder.2's epilogue and of head layer 1's barrier)
    // instead of being held from here on: with the shorter epilogues' schedule they were what that kernel spilled.
    // Every other kernel keeps them in registers (on 16-candidate tiles the late reads cost 0.1 us per launch).
    constexpr bool LATE_SCALES = PRE && PL == X3Q && NT == 4;
    f32x4 bf[NT];
    float s1[NT], s2[NT], u2[NT], uh[NT], sh[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
        bf[ct] = ld4(&sm.xin[(ct * 16 + n) * 16 + 4 * q]);
        if constexpr (LATE_SCALES) {
            s1[ct] = col_scale(sm, ct * 16 + n, 0);
        } else {
            ColScales cs;
            if constexpr (PRE) {
                const f32x4 a = sm.cscl[ct * 16 + n][0];
                cs = ColScales{a.x, a.y, a.z, a.w, sm.cscl[ct * 16 + n][1].x};
            } else {
                cs = split_col_scales(xin_row_absmax(bf[ct]), hs);
            }
            s1[ct] = cs.s1;
            s2[ct] = cs.s2;
            u2[ct] = cs.u2;
            uh[ct] = cs.uh;
            sh[ct] = cs.sh;
        }
    }
    // ---- pose_encoder.0 (9 -> 256) in fp32, one k-group; ReLU, scale, split into the chunk planes
#pragma unroll
    for (int c = 0; c < CPW; ++c) {
        const int Ta = wid * TPW + 2 * c;
        const f32x4 a0 = hs.pe0a[2 * c], a1 = hs.pe0a[2 * c + 1];
        const f32x4 bias0 = hs.pe0b[2 * c], bias1 = hs.pe0b[2 * c + 1];
#pragma unroll
        for (int ct = 0; ct < NP; ++ct) {
            const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
            f16x8 pl[X3P];
            if constexpr (JVP) {   // the tangent tile: no bias, the primal's masks; its own bound (s1 of its eps row)
                constexpr int dt = JVP ? NP : 0;
                const f32x4 pre0 = mfma_kgroup(a0, bf[ct], z) + bias0, pre1 = mfma_kgroup(a1, bf[ct], z) + bias1;
                split3_pair(relu4(pre0), relu4(pre1), s1[ct], pl);
#pragma unroll
                for (int p = 0; p < X3P; ++p) act1h[(((Ta >> 1) * NT + ct) * X3P + p) * 64 + lane] = pl[p];
                split3_pair(mask4(mfma_kgroup(a0, bf[ct + dt], z), pre0), mask4(mfma_kgroup(a1, bf[ct + dt], z), pre1),
                            s1[ct + dt], pl);
#pragma unroll
                for (int p = 0; p < X3P; ++p) act1h[(((Ta >> 1) * NT + ct + dt) * X3P + p) * 64 + lane] = pl[p];
            } else {
                ActPlanes<PL> ap;
                split_act<PL>(relu4(mfma_kgroup(a0, bf[ct], z) + bias0), relu4(mfma_kgroup(a1, bf[ct], z) + bias1), s1[ct], ap);
                store_act<PL, NT>(act1h, Ta >> 1, ct, lane, ap);
            }
        }
    }
    __syncthreads();
    PC_MARK(2);
    // ---- pose_encoder.2 (256 -> 256)
    stream_x3_step<PL, D2, KC_HID + D2, TPW, NT, D2>(W2, T2, act1h, lane, voff, ring2, acc2, cor2);
    PC_MARK(3);
    // head layer 1's first chunks and init rows (head 0), in flight across the pose_encoder.2 epilogue
    f16x8 ringh[DH + 1][TPW][ring_planes<PL>()];
    {
        int TH0[TPW];
#pragma unroll
        for (int t = 0; t < TPW; ++t) TH0[t] = wid * TPW + t;
        stream_x3_step<PL, 0, DH, TPW, NT, DH>(WH, TH0, act2h, lane, voff, ringh, acc2, cor2);
    }
    const __amdgpu_buffer_rsrc_t RP = make_rsrc(pobj, 0x7ffffff0u), RT = make_rsrc(tproj, 3 * HID * 4);
    int vo[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) vo[ct] = obj_of_col[ct * 16 + n] * (3 * HID * 4) + 16 * q;
    f32x4 tpv[TPW], pov[TPW][NP];
    head_x3_init_load<0, NT, TPW, NP>(RP, RT, vo, wid, lane, tpv, pov);
    // the epilogue's planes are made before the alias barrier (a wave that finished its stream early does
    // this VALU work while it waits for the last one) and only written after it (profiles/r4/ab_epi_early.json)
    ActPlanes<PL> pls[CPW][NT];
    if constexpr (LATE_SCALES) {
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            s2[ct] = col_scale(sm, ct * 16 + n, 1);
            u2[ct] = col_scale(sm, ct * 16 + n, 2);
        }
    }
#pragma unroll
    for (int c = 0; c < CPW; ++c) {
        const int Ta = T2[2 * c];
        const f32x4 bias0 = ld4(&sm.pe2b[16 * Ta + 4 * q]), bias1 = ld4(&sm.pe2b[16 * (Ta + 1) + 4 * q]);
#pragma unroll
        for (int ct = 0; ct < NP; ++ct) {
            if constexpr (JVP) {
                constexpr int dt = JVP ? NP : 0;
                const f32x4 pre0 = (acc2[2 * c][ct] + cor2[2 * c][ct]) * u2[ct] + bias0;
                const f32x4 pre1 = (acc2[2 * c + 1][ct] + cor2[2 * c + 1][ct]) * u2[ct] + bias1;
                split3_pair(relu4(pre0), relu4(pre1), s2[ct], pls[c][ct].h);
                split3_pair(mask4((acc2[2 * c][ct + dt] + cor2[2 * c][ct + dt]) * u2[ct + dt], pre0),
                            mask4((acc2[2 * c + 1][ct + dt] + cor2[2 * c + 1][ct + dt]) * u2[ct + dt], pre1),
                            s2[ct + dt], pls[c][ct + dt].h);
            } else {
                split_act<PL>(relu4((acc2[2 * c][ct] + cor2[2 * c][ct]) * u2[ct] + bias0),
                              relu4((acc2[2 * c + 1][ct] + cor2[2 * c + 1][ct]) * u2[ct] + bias1), s2[ct], pls[c][ct]);
            }
        }
    }
    if constexpr (SM::kAliasAct) __syncthreads();   // act2 overwrites act1: all reads done
#pragma unroll
    for (int c = 0; c < CPW; ++c)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
            store_act<PL, NT>(act2h, T2[2 * c] >> 1, ct, lane, pls[c][ct]);
    if constexpr (LATE_SCALES) {   // in front of the barrier, whose wait covers the reads
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            uh[ct] = col_scale(sm, ct * 16 + n, 3);
            sh[ct] = col_scale(sm, ct * 16 + n, 4);
        }
    }
    __syncthreads();
    PC_MARK(4);
    // ---- head layer 1 (pose block 256 -> 3x256) head by head, each followed by its layer-2 partials
    float pv[SM::kRedV];
#pragma unroll
    for (int v = 9 * NT; v < SM::kRedV; ++v) pv[v] = 0.f;
    head_x3_head<0, NT, WV, TPW, DH, JVP, PL>(WH, act2h, RP, RT, vo, sm, uh, sh, wid, lane, ringh, tpv, pov, pv);
    PC_MARK(13);
    head_x3_head<1, NT, WV, TPW, DH, JVP, PL>(WH, act2h, RP, RT, vo, sm, uh, sh, wid, lane, ringh, tpv, pov, pv);
    PC_MARK(14);
    head_x3_head<2, NT, WV, TPW, DH, JVP, PL>(WH, act2h, RP, RT, vo, sm, uh, sh, wid, lane, ringh, tpv, pov, pv);
    PC_MARK(5);
    if constexpr ((3 * NT) % 4 != 0) {
#pragma unroll
        for (int g = 0; g < SM::kRedV / 4; ++g)
            sm.red[4 * g + q][n][wid] = rows_sum_scatter4(pv[4 * g], pv[4 * g + 1], pv[4 * g + 2], pv[4 * g + 3]);
    }
    __syncthreads();
    PC_MARK(6);
}

// The object (row of pobj) of candidate row r; rows past the end take the last row's, which keeps their loads in bounds
__device__ __forceinline__ int obj_of_row(int r, int rows, int kper) { return (r < rows ? r : rows - 1) / kper; }

// The trunk of the form PL (taken from sm): head_trunk for 0, head_trunk_x3 otherwise. hs: load_split_scalars<PL>.
// For the PC step, the ODE stages and the denoise kernel. The evaluation and JVP kernels select their trunk
// themselves: through this wrapper the compiler allocated their registers differently and, in the exact-fp32 JVP
// trunk, contracted other products of the layer-2 sums (which are not under contract(off)), so the divergence lost
// its bits.
template <bool PRE = false, int NT, int WV, int PL>
__device__ __forceinline__ void run_head_trunk(const gp_head_weights& w, const float* pobj, const float* tproj,
                                               const int* obj_of_col,
                                               HeadSmem<NT, WV, PL>& sm, int trace_slot, const SplitScalars& hs) {
    if constexpr (PL != 0)
        head_trunk_x3<NT, WV, PRE>(w, pobj, tproj, obj_of_col, sm, trace_slot, hs);
    else
        head_trunk<NT, WV>(w, pobj, tproj, obj_of_col, sm, trace_slot);
}

// ============================================================================ tile width
#ifndef PC_SPLIT_NT2_MIN
#define PC_SPLIT_NT2_MIN 4097   // rows from which the split kernels take 32-candidate tiles (> 256 tiles of 16)
#endif
#ifndef PC_SPLIT_NT4_MIN
#define PC_SPLIT_NT4_MIN 8193   // ... and 64-candidate tiles (> 256 tiles of 32)
#endif
// Column tiles (16 candidates each) per workgroup of the per-candidate head kernels (PC step, ODE stages).
// exact fp32 (scripts/kbench.py): 16 candidates x 8 waves per workgroup beats 32 x 4 at every size
// (R=25,600: 125 vs 153 us/step): 112 VGPRs leave room for two workgroups per CU, while the 32-wide
// tile needs 373 registers (one wave per SIMD).
// split-f16: each workgroup streams the 1 MB of GEMM weights once per launch whatever its width, so
// wider tiles cut the weight stream per candidate once there are enough tiles. One workgroup per CU
// either way (the LDS of a 32- or 64-candidate tile), so the tile width is the smallest that keeps the
// launch within one pass of the 256 CUs, or the widest above that.
static inline int head_pick_nt(int rows, bool split) {
    if (!split) return 1;
    return rows >= PC_SPLIT_NT4_MIN ? 4 : (rows >= PC_SPLIT_NT2_MIN ? 2 : 1);
}
// Host: f(PL, NT), both std::integral_constant<int, .>, for the trunk form pl and nt column tiles per workgroup.
// A launch site instantiates the exact-fp32 form at 16-candidate tiles only, the f16x3 form at the widths up
// to MAX_NT, and the hybrid form (at the same widths) only where Q8 says it can take it.
template <int MAX_NT = 4, bool Q8 = false, typename F>
static inline void head_dispatch(int pl, int nt, F f) {
    auto widths = [&](auto PL) {
        if constexpr (MAX_NT >= 4)
            if (nt == 4) return f(PL, std::integral_constant<int, 4>{});
        if constexpr (MAX_NT >= 2)
            if (nt == 2) return f(PL, std::integral_constant<int, 2>{});
        return f(PL, std::integral_constant<int, 1>{});
    };
    if (pl == 0) return f(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
    if constexpr (Q8)
        if (pl == X3Q) return widths(std::integral_constant<int, X3Q>{});
    return widths(std::integral_constant<int, X3P>{});
}

// ============================================================================ pose helpers
template <typename T>
__device__ __forceinline__ T tsqrt(T v);
template <>
__device__ __forceinline__ float tsqrt<float>(float v) { return sqrtf(v); }
template <>
__device__ __forceinline__ double tsqrt<double>(double v) { return sqrt(v); }

// normalize_rotation(.., 'rot_matrix') (misc.py:327-344): rotation_6d_to_matrix GS with
// F.normalize's eps 1e-12 (rotation_conversions.py:571-575). The bits are those of the written-out order below,
// which tests/pose_ref.py states operation by operation and oracle.gram_schmidt reproduces -- not torch's: F.normalize's
// vector_norm sums the three squares in another order, and the reference's float32 CPU result differs from this
// one in the last place on 23 % of rows (43 % after the quaternion; tests/test_cpu_pose_edges.py). The clamp is a
// select, so a NaN norm becomes 1e-12 where torch's clamp_min keeps the NaN (the quaternion is NaN either way).
template <typename T>
__device__ __forceinline__ void gram_schmidt6(T* v) {
#pragma clang fp contract(off)
    T n1 = tsqrt<T>((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    n1 = n1 > (T)1e-12 ? n1 : (T)1e-12;
    const T b0 = v[0] / n1, b1 = v[1] / n1, b2 = v[2] / n1;
    const T d = (b0 * v[3] + b1 * v[4]) + b2 * v[5];
    T c0 = v[3] - d * b0, c1 = v[4] - d * b1, c2 = v[5] - d * b2;
    T n2 = tsqrt<T>((c0 * c0 + c1 * c1) + c2 * c2);
    n2 = n2 > (T)1e-12 ? n2 : (T)1e-12;
    v[0] = b0;
    v[1] = b1;
    v[2] = b2;
    v[3] = c0 / n2;
    v[4] = c1 / n2;
    v[5] = c2 / n2;
}

// gram_schmidt6 spread over the four lanes of a row (lane part p: 0 -> v[0:3], 1 -> v[3:6],
// 2 -> translation, untouched; 3 idle). Same operations and order as gram_schmidt6<float>: IEEE division
// and square root on purpose (the hardware's approximate ones would not give the bits of the written-out order
// that tests/pose_ref.py states and the oracle reproduces; tests/test_gpu_pose_edges.py holds both forms to them).
__device__ __forceinline__ void gram_schmidt6_quad(float* v, int p, int lane) {
#pragma clang fp contract(off)
    float n1 = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    n1 = n1 > 1e-12f ? n1 : 1e-12f;
    const float b0 = fdiv(v[0], n1), b1 = fdiv(v[1], n1), b2 = fdiv(v[2], n1);   // meaningful on p == 0
    (void)lane;
    const float B0 = quad_bcast0(b0), B1 = quad_bcast0(b1), B2 = quad_bcast0(b2);
    const float d = (B0 * v[0] + B1 * v[1]) + B2 * v[2];
    float c0 = v[0] - d * B0, c1 = v[1] - d * B1, c2 = v[2] - d * B2;
    float n2 = sqrtf((c0 * c0 + c1 * c1) + c2 * c2);
    n2 = n2 > 1e-12f ? n2 : 1e-12f;
    if (p == 0) {
        v[0] = b0; v[1] = b1; v[2] = b2;
    } else if (p == 1) {
        v[0] = fdiv(c0, n2); v[1] = fdiv(c1, n2); v[2] = fdiv(c2, n2);
    }
}

// matrix_to_quaternion (rotation_conversions.py:102-161) of R = [b1 b2 b1xb2] (columns), input
// already Gram-Schmidt'ed; returns wxyz.
template <typename T>
__device__ __forceinline__ void quat_from_gs(const T* v, T* qo) {
#pragma clang fp contract(off)
    // second GS pass as get_rot_matrix applies rotation_6d_to_matrix again (posenet_agent.py:554)
    T g[6] = {v[0], v[1], v[2], v[3], v[4], v[5]};
    gram_schmidt6<T>(g);
    const T b3x = g[1] * g[5] - g[2] * g[4];
    const T b3y = g[2] * g[3] - g[0] * g[5];
    const T b3z = g[0] * g[4] - g[1] * g[3];
    const T m00 = g[0], m01 = g[3], m02 = b3x;
    const T m10 = g[1], m11 = g[4], m12 = b3y;
    const T m20 = g[2], m21 = g[5], m22 = b3z;
    const T one = (T)1;
    T qa[4] = {((one + m00) + m11) + m22, ((one + m00) - m11) - m22, ((one - m00) + m11) - m22,
               ((one - m00) - m11) + m22};
#pragma unroll
    for (int i = 0; i < 4; ++i) qa[i] = qa[i] > (T)0 ? tsqrt<T>(qa[i]) : (T)0;
    int best = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (qa[i] > qa[best]) best = i;
    T c[4];
    if (best == 0) {
        c[0] = qa[0] * qa[0]; c[1] = m21 - m12; c[2] = m02 - m20; c[3] = m10 - m01;
    } else if (best == 1) {
        c[0] = m21 - m12; c[1] = qa[1] * qa[1]; c[2] = m10 + m01; c[3] = m02 + m20;
    } else if (best == 2) {
        c[0] = m02 - m20; c[1] = m10 + m01; c[2] = qa[2] * qa[2]; c[3] = m12 + m21;
    } else {
        c[0] = m10 - m01; c[1] = m20 + m02; c[2] = m21 + m12; c[3] = qa[3] * qa[3];
    }
    const T den = (T)2 * (qa[best] > (T)0.1 ? qa[best] : (T)0.1);
#pragma unroll
    for (int i = 0; i < 4; ++i) qo[i] = c[i] / den;
}

// Head layer-1 t block for one time value (HT threads): tproj = W1_t . relu(W_te . [sin, cos](GFP(t)) + b_te)
// (scorenet.py:77-88 GaussianFourierProjection + t_encoder, the t columns of the first head layer).
// Writes out[o] for o in [o0, o1) (the caller's slice of the 768-row).
// sum_c W[c * stride] * x[c] over N = CH * L terms as CH interleaved fp32 chains (chain j: c = j, j + CH,
// ...) combined by a pairwise tree -- the accumulation pattern of a vectorised CPU GEMM. A single
// N-term chain is ~sqrt(N) roundings deep; the energy's pose . score sums cancel enough to expose it
// (the 1024-term pts block of head layer 1 was 2x the reference's own fp32 error at R=12,800).
template <int N, int CH>
__device__ __forceinline__ float dot_chains(const float* __restrict__ W, size_t stride, const float* x) {
    static_assert(N % CH == 0 && (CH & (CH - 1)) == 0, "N must be a multiple of the power-of-two CH");
    float p[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) p[j] = 0.f;
#pragma unroll 1
    for (int c0 = 0; c0 < N; c0 += CH) {
#pragma unroll
        for (int j = 0; j < CH; ++j) p[j] = fmaf(W[(size_t)(c0 + j) * stride], x[c0 + j], p[j]);
    }
#pragma unroll
    for (int s = CH / 2; s >= 1; s >>= 1)
#pragma unroll
        for (int j = 0; j < s; ++j) p[j] += p[j + s];
    return p[0];
}

// HOIST64 (diagnostic builds): the hoisted head-1 rows' GEMMs (object block, t_encoder, t block) accumulated in
// float64 and rounded once -- how far the order of those sums moves the T0=1 ODE path (tests/test_gpu_parity.py
// test_ode_t1_calibrated_vs_float64). The Fourier embedding stays the reference's float32 computation.
#ifndef HOIST64
#define HOIST64 0
#endif
template <int N>
__device__ __forceinline__ double dot_f64(const float* __restrict__ W, size_t stride, const float* x) {
    double s = 0.0;   // each fp32 x fp32 product is exact in float64
#pragma unroll 8
    for (int c = 0; c < N; ++c) s = fma((double)W[(size_t)c * stride], (double)x[c], s);
    return s;
}

__device__ __forceinline__ void time_row(const gp_head_weights& w, float t, float* emb, float* tf,
                                         float* __restrict__ out, int o0 = 0, int o1 = 768) {
    const int i = threadIdx.x;
    if (i < 64) {  // x_proj = x[:, None] * W[None, :] * 2 * np.pi (scorenet.py:87)
        const float a = fmul(fmul(fmul(t, w.gfp_w[i]), 2.0f), 3.14159265358979323846f);
        emb[i] = sinf(a);
        emb[64 + i] = cosf(a);
    }
    __syncthreads();
#if HOIST64
    if (i < 128) tf[i] = fmaxf((float)(dot_f64<128>(w.te_w_t + i, 128, emb) + (double)w.te_b[i]), 0.f);
    __syncthreads();
    for (int o = o0 + i; o < o1; o += HT) out[o] = (float)dot_f64<128>(w.h1t_t + o, 768, tf);
#else
    if (i < 128) tf[i] = fmaxf(dot_chains<128, 16>(w.te_w_t + i, 128, emb) + w.te_b[i], 0.f);
    __syncthreads();
    for (int o = o0 + i; o < o1; o += HT) out[o] = dot_chains<128, 16>(w.h1t_t + o, 768, tf);
#endif
}
