// Candidate ranking and pose aggregation on device (one workgroup of 64 threads per object).
//
// Reference: sort_poses_by_energy (networks/reward.py:131-155), aggregate_pose
// (runners/evaluation_single.py:160-219), average_quaternion_batch (utils/misc.py:295-317),
// rotation_6d_to_matrix / matrix_to_quaternion / quaternion_to_matrix
// (utils/transforms/rotation_conversions.py:41-161,556-577) and sklearn DBSCAN(eps, min_samples)
// applied with its default Euclidean metric to the ROWS of the quaternion distance matrix
// (SURVEY F9). The reference runs this as a host loop over objects with .cpu().numpy() round trips.
//
//  1. ranks by descending rotation / translation energy (ties -> lower candidate index);
//  2. top `retain` rotations (by rotation energy) and translations (by translation energy);
//  3. quaternion (wxyz) of each kept rotation, sign-oriented weighted outer-product mean, top
//     eigenvector by cyclic Jacobi on the 4x4 in fp64 (the reference calls fp32 eigh);
//  4. optional DBSCAN over the kept set (core: >= min_samples neighbours within eps incl. itself;
//     clusters grown depth-first from core points in index order), re-average of the largest
//     cluster (first label on count ties, numpy argmax);
//  5. mean translation, 4x4 [R t; 0 1].
//
// gp_rank_aggregate_modes is the same launch with step 4 finished: every cluster's average, count, mean energy
// and spread (pose hypotheses), and the slot nearest to a previous rotation. The two kernels share their body
// (gp_aggregate_body.h).
#include "gp_common.h"

constexpr int AGG_THREADS = 64;
constexpr int AGG_MAXK = 1024;
constexpr int AGG_MAXKEEP = 128;

// normalize_rotation -> rotation_6d_to_matrix -> matrix_to_quaternion, fp32 (as the reference).
__device__ __forceinline__ void rot6_to_quat(const float* v, float* q) {
#pragma clang fp contract(off)
    float n1 = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    n1 = n1 > 1e-12f ? n1 : 1e-12f;
    const float b0 = v[0] / n1, b1 = v[1] / n1, b2 = v[2] / n1;
    const float d = (b0 * v[3] + b1 * v[4]) + b2 * v[5];
    float c0 = v[3] - d * b0, c1 = v[4] - d * b1, c2 = v[5] - d * b2;
    float n2 = sqrtf((c0 * c0 + c1 * c1) + c2 * c2);
    n2 = n2 > 1e-12f ? n2 : 1e-12f;
    c0 /= n2; c1 /= n2; c2 /= n2;
    const float b3x = b1 * c2 - b2 * c1, b3y = b2 * c0 - b0 * c2, b3z = b0 * c1 - b1 * c0;
    // matrix columns b1, b2, b3 (get_rot_matrix permutes rotation_6d_to_matrix's rows)
    const float m00 = b0, m01 = c0, m02 = b3x, m10 = b1, m11 = c1, m12 = b3y, m20 = b2, m21 = c2, m22 = b3z;
    float qa[4] = {((1.f + m00) + m11) + m22, ((1.f + m00) - m11) - m22, ((1.f - m00) + m11) - m22,
                   ((1.f - m00) - m11) + m22};
#pragma unroll
    for (int i = 0; i < 4; ++i) qa[i] = qa[i] > 0.f ? sqrtf(qa[i]) : 0.f;
    int best = 0;
    float qb = qa[0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (qa[i] > qb) { qb = qa[i]; best = i; }
    float c[4];
    if (best == 0) { c[0] = qa[0] * qa[0]; c[1] = m21 - m12; c[2] = m02 - m20; c[3] = m10 - m01; }
    else if (best == 1) { c[0] = m21 - m12; c[1] = qa[1] * qa[1]; c[2] = m10 + m01; c[3] = m02 + m20; }
    else if (best == 2) { c[0] = m02 - m20; c[1] = m10 + m01; c[2] = qa[2] * qa[2]; c[3] = m12 + m21; }
    else { c[0] = m10 - m01; c[1] = m20 + m02; c[2] = m21 + m12; c[3] = qa[3] * qa[3]; }
    const float den = 2.f * (qb > 0.1f ? qb : 0.1f);
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = c[i] / den;
}

// Top eigenvector of a symmetric 4x4 (cyclic Jacobi, fp64), oriented so that w >= 0 is kept and
// w <= 0 flipped exactly as ((q[0] > 0) - 0.5) * 2 * q does.
__device__ void top_eigvec4(double A[4][4], float* out) {
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0;
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int r = p + 1; r < 4; ++r) off += A[p][r] * A[p][r];
        const double diag = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2] + A[3][3] * A[3][3];
        if (off <= 1e-36 * diag || off < 1e-300) break;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int r = p + 1; r < 4; ++r) {
                if (A[p][r] == 0.0) continue;
                const double theta = (A[r][r] - A[p][p]) / (2.0 * A[p][r]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; ++k) {  // A <- J^T A J
                    const double akp = A[k][p], akr = A[k][r];
                    A[k][p] = c * akp - s * akr;
                    A[k][r] = s * akp + c * akr;
                }
                for (int k = 0; k < 4; ++k) {
                    const double apk = A[p][k], ark = A[r][k];
                    A[p][k] = c * apk - s * ark;
                    A[r][k] = s * apk + c * ark;
                }
                for (int k = 0; k < 4; ++k) {
                    const double vkp = V[k][p], vkr = V[k][r];
                    V[k][p] = c * vkp - s * vkr;
                    V[k][r] = s * vkp + c * vkr;
                }
            }
    }
    // column of the largest eigenvalue (register selects, no dynamic indexing)
    double lam = A[0][0], v[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int c = 1; c < 4; ++c)
        if (A[c][c] > lam) {
            lam = A[c][c];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = V[i][c];
        }
    const double nrm = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
    const double sgn = (v[0] / nrm > 0.0) ? 1.0 : -1.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = (float)(sgn * v[i] / nrm);
}

// Does candidate (b, j) come before (a, i) in torch.sort(descending=True) order? NaN sorts as the
// largest value (torch's comparator), equal keys (NaN with NaN too) keep the lower index first.
__device__ __forceinline__ bool precedes(float b, int j, float a, int i) {
    const bool an = a != a, bn = b != b;
    if (an || bn) return bn && (!an || j < i);
    return b > a || (b == a && j < i);
}

struct AggSmem {
    int rank_rot[AGG_MAXK];
    int rank_tr[AGG_MAXK];
    int ord_rot[AGG_MAXKEEP];
    int ord_tr[AGG_MAXKEEP];
    float q[AGG_MAXKEEP][4];
    float qo[AGG_MAXKEEP][4];   // w-oriented copies
    float D[AGG_MAXKEEP][AGG_MAXKEEP + 1];
    unsigned char adj[AGG_MAXKEEP][AGG_MAXKEEP];   // |D_i - D_j|_2 <= eps
    int ncount[AGG_MAXKEEP];
    int label[AGG_MAXKEEP];
    int stack[AGG_MAXKEEP];
    float qavg[4];
};

// Pose hypotheses (gp_rank_aggregate_modes): every DBSCAN cluster of the kept rotations, not only the
// largest. The LDS of the modes kernel is AggSmem followed by ModeSmem.
constexpr int AGG_MAXMODES = 8;

struct ModeSmem {
    int nlab;                        // L: clusters DBSCAN found (0 without clustering)
    int lcount[AGG_MAXKEEP];         // members per label
    int slot_label[AGG_MAXMODES];    // label behind slot m (descending count, ties -> lower label)
    float mq[AGG_MAXMODES][4];       // mode quaternions
    float mt[AGG_MAXMODES][3];       // mode translations
};

struct ModeArgs {
    int max_modes;
    const float* prev_rot;   // (B,3,3) or null
    float* mode_pose;        // (B,M,4,4)
    int* mode_count;         // (B,M)
    float* mode_energy;      // (B,M)
    float* mode_spread;      // (B,M)
    int* n_clusters;         // (B,)
    int* noise_count;        // (B,)
    int* nearest;            // (B,)
};

// Per-mode means that have no counterpart in the reference's aggregate: the members' own translations,
// their rotation energies and 1 - <q_r, q_mode>^2, each an fp32 sum in rank order over the count.
// sel < 0: every kept candidate is a member (no cluster: the reference's fallback).
__device__ __forceinline__ void mode_means(const AggSmem& sm, const float* P, const float* E, int keep, int sel,
                                           int count, const float* qm, float* t, float* en, float* spread) {
#pragma clang fp contract(off)
    float t0 = 0.f, t1 = 0.f, t2 = 0.f, e = 0.f, s = 0.f;
    for (int r = 0; r < keep; ++r) {
        if (sel >= 0 && sm.label[r] != sel) continue;
        const int c = sm.ord_rot[r];
        t0 += P[9 * c + 6];
        t1 += P[9 * c + 7];
        t2 += P[9 * c + 8];
        e += E[2 * c];
        const float dot = ((sm.q[r][0] * qm[0] + sm.q[r][1] * qm[1]) + sm.q[r][2] * qm[2]) + sm.q[r][3] * qm[3];
        s += 1.f - dot * dot;
    }
    const float n = (float)count;
    t[0] = t0 / n;
    t[1] = t1 / n;
    t[2] = t2 / n;
    *en = e / n;
    *spread = s / n;
}

__global__ __launch_bounds__(AGG_THREADS) void rank_aggregate_kernel(
    const float* __restrict__ poses, const float* __restrict__ energy, int K, int keep, int clustering,
    float eps, int min_samples, float* __restrict__ agg, float* __restrict__ sorted_pose,
    float* __restrict__ sorted_energy) {
#define AGG_MODES 0
#include "gp_aggregate_body.h"
#undef AGG_MODES
}

__global__ __launch_bounds__(AGG_THREADS) void rank_aggregate_modes_kernel(
    const float* __restrict__ poses, const float* __restrict__ energy, int K, int keep, int clustering,
    float eps, int min_samples, float* __restrict__ agg, float* __restrict__ sorted_pose,
    float* __restrict__ sorted_energy, ModeArgs ma) {
#define AGG_MODES 1
#include "gp_aggregate_body.h"
#undef AGG_MODES
}

extern "C" int gp_rank_aggregate(const float* poses, const float* energy, int b, int k, int retain, int clustering,
                                 float eps, int min_samples, float* aggregated, float* sorted_pose,
                                 float* sorted_energy, hipStream_t stream) {
    GP_REQUIRE(b == 0 || (poses && energy && aggregated), "rank_aggregate: null pointer");
    GP_REQUIRE(b >= 0 && k >= 1 && k <= AGG_MAXK, "rank_aggregate: need 1 <= k <= %d (k=%d)", AGG_MAXK, k);
    GP_REQUIRE(retain >= 1 && retain <= k && retain <= AGG_MAXKEEP, "rank_aggregate: need 1 <= retain <= min(k, %d)",
               AGG_MAXKEEP);
    GP_REQUIRE(!clustering || min_samples >= 1, "rank_aggregate: DBSCAN needs min_samples >= 1");
    if (!b) return GP_OK;
    const size_t lds = sizeof(AggSmem);
    if (lds > 160 * 1024) {
        gp_set_error("rank_aggregate: LDS %zu", lds);
        return GP_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(rank_aggregate_kernel, dim3(b), dim3(AGG_THREADS), lds, stream, poses, energy, k, retain,
                       clustering, eps, min_samples, aggregated, sorted_pose, sorted_energy);
    return gp_check_launch("rank_aggregate_kernel");
}

extern "C" int gp_rank_aggregate_modes(const float* poses, const float* energy, int b, int k, int retain,
                                       int clustering, float eps, int min_samples, int max_modes,
                                       const float* prev_rot, float* aggregated, float* sorted_pose,
                                       float* sorted_energy, float* mode_pose, int* mode_count, float* mode_energy,
                                       float* mode_spread, int* n_clusters, int* noise_count, int* nearest,
                                       hipStream_t stream) {
    GP_REQUIRE(max_modes >= 1 && max_modes <= AGG_MAXMODES, "rank_aggregate_modes: need 1 <= max_modes <= %d (%d)",
               AGG_MAXMODES, max_modes);
    GP_REQUIRE(b == 0 || (poses && energy && aggregated), "rank_aggregate_modes: null pointer");
    GP_REQUIRE(b == 0 || (mode_pose && mode_count && mode_energy && mode_spread && n_clusters && noise_count && nearest),
               "rank_aggregate_modes: null mode output");
    GP_REQUIRE(b >= 0 && k >= 1 && k <= AGG_MAXK, "rank_aggregate_modes: need 1 <= k <= %d (k=%d)", AGG_MAXK, k);
    GP_REQUIRE(retain >= 1 && retain <= k && retain <= AGG_MAXKEEP,
               "rank_aggregate_modes: need 1 <= retain <= min(k, %d)", AGG_MAXKEEP);
    GP_REQUIRE(!clustering || min_samples >= 1, "rank_aggregate_modes: DBSCAN needs min_samples >= 1");
    if (!b) return GP_OK;
    const size_t lds = sizeof(AggSmem) + sizeof(ModeSmem);
    if (lds > 160 * 1024) {
        gp_set_error("rank_aggregate_modes: LDS %zu", lds);
        return GP_ERR_UNSUPPORTED;
    }
    const ModeArgs ma{max_modes, prev_rot, mode_pose, mode_count, mode_energy, mode_spread, n_clusters, noise_count,
                      nearest};
    hipLaunchKernelGGL(rank_aggregate_modes_kernel, dim3(b), dim3(AGG_THREADS), lds, stream, poses, energy, k, retain,
                       clustering, eps, min_samples, aggregated, sorted_pose, sorted_energy, ma);
    return gp_check_launch("rank_aggregate_modes_kernel");
}

// ============================================================================ stage glue
// process_batch's pts_center (datasets_omni6dpose.py:746-752: zero_mean = mean(pts[:, :, :3], 1)).
// One workgroup per object; per-thread strided sums over points, then a fixed-order tree.
__global__ __launch_bounds__(256) void points_mean_kernel(const float* __restrict__ pts, int n, int c,
                                                          float* __restrict__ out) {
    __shared__ float red[3][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    const float* p = pts + (size_t)b * n * c;
    for (int i = tid; i < n; i += 256) {
        s0 += ld1(p + (size_t)i * c + 0);
        s1 += ld1(p + (size_t)i * c + 1);
        s2 += ld1(p + (size_t)i * c + 2);
    }
    red[0][tid] = s0;
    red[1][tid] = s1;
    red[2][tid] = s2;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
            red[0][tid] += red[0][tid + st];
            red[1][tid] += red[1][tid + st];
            red[2][tid] += red[2][tid + st];
        }
        __syncthreads();
    }
    if (tid < 3) out[(size_t)b * 3 + tid] = fdiv(red[tid][0], (float)n);
}

extern "C" int gp_points_mean(const float* pts, int b, int n, int c, float* out, hipStream_t stream) {
    GP_REQUIRE(b >= 0 && n >= 1 && c >= 3 && (b == 0 || (pts && out)), "points_mean: bad arguments");
    if (!b) return GP_OK;
    hipLaunchKernelGGL(points_mean_kernel, dim3(b), dim3(256), 0, stream, pts, n, c, out);
    return gp_check_launch("points_mean_kernel");
}

// inference_scale without a ScaleNet checkpoint (evaluation_single.py:233-252): the points in the
// aggregated object frame, q = R^T (p - t), and length = 2 max_n |q| per axis. Max is
// order-independent, so the result depends only on the per-point arithmetic.
__global__ __launch_bounds__(256) void bbox_length_kernel(const float* __restrict__ pcl, int n, int c,
                                                          const float* __restrict__ pose, float* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ float red[3][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* P = pose + (size_t)b * 16;
    const float r00 = P[0], r01 = P[1], r02 = P[2], t0 = P[3];
    const float r10 = P[4], r11 = P[5], r12 = P[6], t1 = P[7];
    const float r20 = P[8], r21 = P[9], r22 = P[10], t2 = P[11];
    float m0 = 0.f, m1 = 0.f, m2 = 0.f;
    const float* p = pcl + (size_t)b * n * c;
    for (int i = tid; i < n; i += 256) {
        const float d0 = ld1(p + (size_t)i * c) - t0, d1 = ld1(p + (size_t)i * c + 1) - t1, d2 = ld1(p + (size_t)i * c + 2) - t2;
        // bmm(R^T, d): row j of R^T is column j of R
        m0 = fmaxf(m0, fabsf((r00 * d0 + r10 * d1) + r20 * d2));
        m1 = fmaxf(m1, fabsf((r01 * d0 + r11 * d1) + r21 * d2));
        m2 = fmaxf(m2, fabsf((r02 * d0 + r12 * d1) + r22 * d2));
    }
    red[0][tid] = m0;
    red[1][tid] = m1;
    red[2][tid] = m2;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
            red[0][tid] = fmaxf(red[0][tid], red[0][tid + st]);
            red[1][tid] = fmaxf(red[1][tid], red[1][tid + st]);
            red[2][tid] = fmaxf(red[2][tid], red[2][tid + st]);
        }
        __syncthreads();
    }
    if (tid < 3) out[(size_t)b * 3 + tid] = red[tid][0] * 2.0f;
}

extern "C" int gp_bbox_length(const float* pcl, int b, int n, int c, const float* pose, float* length,
                              hipStream_t stream) {
    GP_REQUIRE(b >= 0 && n >= 1 && c >= 3 && (b == 0 || (pcl && pose && length)), "bbox_length: bad arguments");
    if (!b) return GP_OK;
    hipLaunchKernelGGL(bbox_length_kernel, dim3(b), dim3(256), 0, stream, pcl, n, c, pose, length);
    return gp_check_launch("bbox_length_kernel");
}
