// The frozen DINOv3 ViT-S+/16 backbone of --dino pointwise (posenet.py:56-62, 138-144) for gfx950:
// get_intermediate_layers(roi_rgb, n=[2, 6, 11], reshape=False, norm=True, return_class_token=False).
//   * patch embedding: Conv2d(3, 384, 16, stride 16) as an implicit-im2col GEMM on exact-fp32 MFMA that reads
//     roi_rgb (B, 3, H, W) in place (a lane's float4 k-slice is 4 consecutive pixels of one image row);
//   * residual + LayerNorm: h += r (pre-norm: the sum is kept), y = LN(h), max |y| per row for a split consumer;
//     the same kernel applies the final norm and drops the 5 prefix tokens for the three outputs;
//   * attention: 6 heads x 64, RoPE applied to the patch tokens' q and k as they are loaded, flash-style
//     (mha_kernel's scheme: S^T = K Q^T, online softmax, O^T += V^T P^T on v_mfma_f32_16x16x4_f32), the key tail
//     masked, so no (B, 6, n, n) buffer exists;
//   * linears: gp_linear_split (three f16 MFMA products, fp32 accumulation; the residual add and SwiGLU are its
//     epilogues 4 and 5) or gp_linear (exact fp32) with the residual left to the next LayerNorm launch.
// Activations are token-major (rows, C) fp32; the batch runs in chunks of images that fit the workspace.
#include <math.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "gp_common.h"
#include "gp_head.h"   // rows_max

namespace {

constexpr int DN_THREADS = 256;
constexpr int DN_D = 384, DN_HEADS = 6, DN_HD = 64, DN_PREFIX = 5, DN_BLOCKS = 12, DN_HID = 1536;
constexpr int DN_PATCH = 16, DN_PK = 3 * DN_PATCH * DN_PATCH;   // 768
constexpr int DN_MAX_PATCHES = 1024;
// token rows of one chunk: 85 row blocks of 256, so that the n = 384 split GEMMs (proj, w3: 3 column blocks,
// one workgroup per CU) launch 255 workgroups, one wave of the 256 CUs, and the wider ones whole multiples
constexpr int DN_CHUNK_ROWS = 85 * 256;
constexpr float DN_EPS = 1e-5f;

// ============================================================================ prefix tokens
// h[img, t, :] = cls (t = 0) or storage_tokens[t - 1] (t = 1..4); one float4 per thread
__global__ __launch_bounds__(DN_THREADS) void dino_prefix_kernel(const float* __restrict__ cls,
                                                                  const float* __restrict__ storage, int imgs, int n,
                                                                  float* __restrict__ h) {
    const int e = blockIdx.x * DN_THREADS + threadIdx.x;
    constexpr int PER = DN_PREFIX * DN_D / 4;
    if (e >= imgs * PER) return;
    const int img = e / PER, f = e - img * PER, t = f / (DN_D / 4), c = 4 * (f - t * (DN_D / 4));
    const f32x4 v = t == 0 ? ld4(cls + c) : ld4(storage + (size_t)(t - 1) * DN_D + c);
    st4(h + ((size_t)img * n + t) * DN_D + c, v);
}

// ============================================================================ patch embedding
// h[img, 5 + p, o] = sum_k patch(img, p)[k] w[o, k] + bias[o], k = c * 256 + ky * 16 + kx. gemm_nt_body's wave
// layout (4 waves as 2 patch tiles x 2 output groups, a wave owns 2 patch tiles x 4 output tiles of 16): the
// 16-deep k-group g is image row ky = g % 16 of channel g / 16, and lane (q, r) reads its pixels 4q .. 4q + 3.
__global__ __launch_bounds__(DN_THREADS) void dino_patch_embed_kernel(const float* __restrict__ rgb, int imgs, int H,
                                                                       int W, const float* __restrict__ w,
                                                                       const float* __restrict__ bias,
                                                                       float* __restrict__ h) {
    constexpr int TM = 2, TN = 4;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int q = lane >> 4, r = lane & 15;
    const int wp = W / DN_PATCH, np = (H / DN_PATCH) * wp, m = imgs * np, n = np + DN_PREFIX;
    const int row0 = blockIdx.x * (32 * TM) + (wid & 1) * (16 * TM);
    const int ot0 = blockIdx.y * (2 * TN) + (wid >> 1) * TN;
    const float* xp[TM];
    const float* wq[TN];
#pragma unroll
    for (int t = 0; t < TM; ++t) {
        const int row = min(row0 + 16 * t + r, m - 1), img = row / np, p = row - img * np;
        const int pi = p / wp, pj = p - pi * wp;
        xp[t] = rgb + ((size_t)img * 3 * H + (size_t)pi * DN_PATCH) * W + pj * DN_PATCH + 4 * q;
    }
#pragma unroll
    for (int u = 0; u < TN; ++u) wq[u] = w + (size_t)(16 * (ot0 + u) + r) * DN_PK + 4 * q;
    f32x4 acc[TN][TM];
#pragma unroll
    for (int u = 0; u < TN; ++u)
#pragma unroll
        for (int t = 0; t < TM; ++t) acc[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    constexpr int KG = DN_PK / 16;   // 48
    for (int g = 0; g < KG; ++g) {
        const size_t xo = ((size_t)(g >> 4) * H + (g & 15)) * W;   // channel g / 16, patch row g % 16
        f32x4 xa[TM], wa[TN];
#pragma unroll
        for (int t = 0; t < TM; ++t) xa[t] = ld4(xp[t] + xo);
#pragma unroll
        for (int u = 0; u < TN; ++u) wa[u] = ld4(wq[u] + 16 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int u = 0; u < TN; ++u)
#pragma unroll
                for (int t = 0; t < TM; ++t) acc[u][t] = mfma4(wa[u][j], xa[t][j], acc[u][t]);
    }
#pragma unroll
    for (int u = 0; u < TN; ++u) {
        const int o = 16 * (ot0 + u) + 4 * q;
        const f32x4 bv = ld4(bias + o);
#pragma unroll
        for (int t = 0; t < TM; ++t) {
            const int row = row0 + 16 * t + r;
            if (row >= m) continue;
            const int img = row / np, p = row - img * np;
            st4(h + ((size_t)img * n + DN_PREFIX + p) * DN_D + o, acc[u][t] + bv);
        }
    }
}

// ============================================================================ residual + LayerNorm
// One wave per row of 384: h += r (r != null; h is written back), y = LN(h) * gamma + beta, ymax[row] = max |y|.
// drop > 0: rows are (image, token) with n tokens an image; tokens < drop are not written and the others land
// compacted at y[(image * (n - drop) + token - drop)] (the backbone's outputs).
__global__ __launch_bounds__(DN_THREADS) void dino_add_ln_kernel(float* __restrict__ h, const float* __restrict__ r,
                                                                  int m, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta,
                                                                  float* __restrict__ y, float* __restrict__ ymax,
                                                                  int n, int drop) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (DN_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= m) return;   // whole waves leave together
    float* hr = h + (size_t)row * DN_D;
    const bool two = lane < (DN_D / 4 - 64);   // 96 float4 a row: lanes 0..31 hold a second one
    const int c0 = 4 * lane, c1 = 4 * (lane + 64);
    f32x4 v0 = ld4(hr + c0), v1 = two ? ld4(hr + c1) : f32x4{0.f, 0.f, 0.f, 0.f};
    if (r) {
        const float* rr = r + (size_t)row * DN_D;
        v0 += ld4(rr + c0);
        st4(hr + c0, v0);
        if (two) {
            v1 += ld4(rr + c1);
            st4(hr + c1, v1);
        }
    }
    size_t yrow = row;
    if (drop > 0) {
        const int img = row / n, t = row - img * n;
        if (t < drop) return;
        yrow = (size_t)img * (n - drop) + (t - drop);
    }
    const float s = ((v0.x + v0.y) + (v0.z + v0.w)) + ((v1.x + v1.y) + (v1.z + v1.w));
    const float mean = wave_sum(s) / (float)DN_D;
    const f32x4 u0 = v0 - mean, u1 = two ? v1 - mean : f32x4{0.f, 0.f, 0.f, 0.f};
    const float s2 = ((u0.x * u0.x + u0.y * u0.y) + (u0.z * u0.z + u0.w * u0.w)) +
                     ((u1.x * u1.x + u1.y * u1.y) + (u1.z * u1.z + u1.w * u1.w));
    const float rstd = 1.0f / sqrtf(wave_sum(s2) / (float)DN_D + DN_EPS);
    float* yr = y + yrow * DN_D;
    const f32x4 o0 = (u0 * rstd) * ld4(gamma + c0) + ld4(beta + c0);
    float mx = fmaxf(fmaxf(fabsf(o0.x), fabsf(o0.y)), fmaxf(fabsf(o0.z), fabsf(o0.w)));
    st4(yr + c0, o0);
    if (two) {
        const f32x4 o1 = (u1 * rstd) * ld4(gamma + c1) + ld4(beta + c1);
        mx = fmaxf(mx, fmaxf(fmaxf(fabsf(o1.x), fabsf(o1.y)), fmaxf(fabsf(o1.z), fabsf(o1.w))));
        st4(yr + c1, o1);
    }
    if (ymax) {
        mx = rows_max(row16_max(mx));
        if (lane == 0) ymax[row] = mx;
    }
}

// ============================================================================ SwiGLU (exact-fp32 path)
// z (m, 3072) with 16-wide tiles paired (gate, up) -> g (m, 1536) = silu(gate) * up
__global__ __launch_bounds__(DN_THREADS) void dino_swiglu_kernel(const float* __restrict__ z, size_t total4,
                                                                  float* __restrict__ g) {
    const size_t e = (size_t)blockIdx.x * DN_THREADS + threadIdx.x;
    if (e >= total4) return;
    const size_t row = e / (DN_HID / 4);
    const int c = 4 * (int)(e - row * (DN_HID / 4));
    const float* zr = z + row * (2 * DN_HID) + 32 * (c >> 4) + (c & 15);
    const f32x4 a = ld4(zr), b = ld4(zr + 16);
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = a[i] / (1.0f + expf(-a[i])) * b[i];
    st4(g + row * DN_HID + c, v);
}

// ============================================================================ attention
// mha_kernel's flash scheme (gp_fusion.hip) for 6 heads of 64 with RoPE: a workgroup = 64 queries (4 waves x 16)
// of one (image, head); keys in LDS chunks of 64 (K row-major, V transposed). Tokens >= 5 (the patches) have
// q and k rotated as they are loaded: x' = x cos + rotate_half(x) sin with the patch's table row [cos(32) | sin(32)],
// dims d and d ^ 32 being partners. Keys >= n are zero in LDS and masked to -inf; queries >= n read row n - 1 and
// store nothing.
__device__ __forceinline__ f32x4 dino_rope4(const float* __restrict__ row, int c, const float* __restrict__ tab) {
#pragma clang fp contract(off)
    const f32x4 a = ld4(row + c), b = ld4(row + (c ^ 32));
    const f32x4 cs = ld4(tab + (c & 31)), sn = ld4(tab + 32 + (c & 31));
    const f32x4 rot = c < 32 ? -b : b;
    return a * cs + rot * sn;
}

__global__ __launch_bounds__(DN_THREADS) void dino_attention_kernel(const float* __restrict__ qkv,
                                                                     const float* __restrict__ rope, int n, int nqb,
                                                                     float* __restrict__ out,
                                                                     unsigned* __restrict__ ymax) {
    constexpr int NG = DN_HD / 16;   // 4
    constexpr int KC = 64, KS = DN_HD + 4, VS = KC + 4;
    __shared__ __attribute__((aligned(16))) float ks[KC * KS];
    __shared__ __attribute__((aligned(16))) float vt[DN_HD * VS];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int qg = lane >> 4, nl = lane & 15;
    const int t = blockIdx.x;
    const int qb = t % nqb, hb = t / nqb, hh = hb % DN_HEADS, b = hb / DN_HEADS;
    constexpr size_t ld = 3 * DN_D;
    const float* base = qkv + (size_t)b * n * ld + hh * DN_HD;
    const int i = qb * 64 + wid * 16 + nl;
    const int ii = i < n ? i : n - 1;
    f32x4 qf[NG], o[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int c = 16 * g + 4 * qg;
        const float* row = base + (size_t)ii * ld;
        qf[g] = ii >= DN_PREFIX ? dino_rope4(row, c, rope + (size_t)(ii - DN_PREFIX) * 64) : ld4(row + c);
        o[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    constexpr float inv = 0.125f;   // 1 / sqrt(64)
    float m = -INFINITY, lsum = 0.f;
    for (int c0 = 0; c0 < n; c0 += KC) {
        const int kn = min(KC, n - c0), k16 = (kn + 15) & ~15;
        __syncthreads();
        for (int e = threadIdx.x; e < k16 * (DN_HD / 4); e += DN_THREADS) {
            const int j = e / (DN_HD / 4), c = 4 * (e - j * (DN_HD / 4));
            f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
            if (j < kn) {
                const int tok = c0 + j;
                const float* row = base + (size_t)tok * ld;
                kv = tok >= DN_PREFIX ? dino_rope4(row + DN_D, c, rope + (size_t)(tok - DN_PREFIX) * 64)
                                      : ld4(row + DN_D + c);
                vv = ld4(row + 2 * DN_D + c);
            }
            st4(ks + j * KS + c, kv);
            vt[(c + 0) * VS + j] = vv.x;
            vt[(c + 1) * VS + j] = vv.y;
            vt[(c + 2) * VS + j] = vv.z;
            vt[(c + 3) * VS + j] = vv.w;
        }
        __syncthreads();
        const int nt = k16 >> 4;   // 16-key tiles of this chunk (1..4)
        f32x4 s[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            s[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (u < nt) {
                const float* kr = ks + (16 * u + nl) * KS + 4 * qg;
#pragma unroll
                for (int g = 0; g < NG; ++g) s[u] = mfma_kgroup(ld4(kr + 16 * g), qf[g], s[u]);
            }
        }
        float bmax = -INFINITY;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j0 = c0 + 16 * u + 4 * qg;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[u][r] = (u < nt && j0 + r < n) ? s[u][r] * inv : -INFINITY;
                bmax = fmaxf(bmax, s[u][r]);
            }
        }
        const float mn = fmaxf(m, rows_max(bmax));   // finite: key c0 < n is in every chunk
        const float alpha = expf(m - mn);
        m = mn;
        float ps = 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[u][r] = expf(s[u][r] - mn);
                ps += s[u][r];
            }
        lsum = lsum * alpha + ps;
#pragma unroll
        for (int g = 0; g < NG; ++g) o[g] *= alpha;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (u < nt) {
                const float* vr = vt + nl * VS + 16 * u + 4 * qg;
#pragma unroll
                for (int g = 0; g < NG; ++g) o[g] = mfma_kgroup(ld4(vr + 16 * g * VS), s[u], o[g]);
            }
    }
    const float rl = 1.0f / rows_sum(lsum);
    float mx = 0.f;
    if (i < n) {
        float* op = out + ((size_t)b * n + i) * DN_D + hh * DN_HD;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const f32x4 v = o[g] * rl;
            mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
            st4(op + 16 * g + 4 * qg, v);
        }
    }
    if (ymax) {   // the token's max |out| over this head, merged over the 6 heads' workgroups
        mx = rows_max(mx);
        if (qg == 0 && i < n) atomicMax(ymax + (size_t)b * n + i, __float_as_uint(mx));
    }
}

// ============================================================================ workspace
size_t dn_align(size_t floats) { return (floats + 63) & ~(size_t)63; }
struct DinoLayout {
    size_t h, y, qkv, att, r, g, u, mx, total;   // float offsets; mx: 3 row-max vectors
};
DinoLayout dino_layout(int imgs, int n) {
    const size_t m = (size_t)imgs * n;
    DinoLayout L;
    size_t o = 0;
    L.h = o;   o += dn_align(m * DN_D);
    L.y = o;   o += dn_align(m * DN_D);
    L.qkv = o; o += dn_align(m * 3 * DN_D);
    L.att = o; o += dn_align(m * DN_D);
    L.r = o;   o += dn_align(m * DN_D);
    L.g = o;   o += dn_align(m * DN_HID);
    L.u = o;   o += dn_align(m * 2 * DN_HID);
    L.mx = o;  o += 3 * dn_align(m);
    L.total = o;
    return L;
}
bool dino_shape_ok(int b, int h, int w) {
    return b >= 1 && h >= DN_PATCH && w >= DN_PATCH && h % DN_PATCH == 0 && w % DN_PATCH == 0 &&
           (long long)(h / DN_PATCH) * (w / DN_PATCH) <= DN_MAX_PATCHES;
}
int dino_chunk_cap(int b, int n) { return std::min(b, std::max(1, DN_CHUNK_ROWS / n)); }

}   // namespace

extern "C" size_t gp_dino_workspace_size(int b, int h, int w) {
    if (!dino_shape_ok(b, h, w)) return 0;
    const int n = (h / DN_PATCH) * (w / DN_PATCH) + DN_PREFIX;
    return sizeof(float) * dino_layout(dino_chunk_cap(b, n), n).total;
}

extern "C" int gp_dino_rope_table(const float* periods_host, int hp, int wp, float* table, hipStream_t st) {
    GP_REQUIRE(table && hp >= 1 && wp >= 1 && (long long)hp * wp <= DN_MAX_PATCHES,
               "dino_rope_table: null table or grid %d x %d (1..%d patches)", hp, wp, DN_MAX_PATCHES);
    double per[16];
    for (int k = 0; k < 16; ++k) {
        per[k] = periods_host ? (double)periods_host[k] : pow(100.0, k / 16.0);
        GP_REQUIRE(std::isfinite(per[k]) && per[k] > 0.0, "dino_rope_table: period %d is not a positive finite number", k);
    }
    std::vector<float> tab((size_t)hp * wp * 64);
    const double two_pi = 6.283185307179586476925286766559;
    for (int i = 0; i < hp; ++i)
        for (int j = 0; j < wp; ++j) {
            float* row = tab.data() + ((size_t)i * wp + j) * 64;
            const double ch = 2.0 * ((i + 0.5) / hp) - 1.0, cw = 2.0 * ((j + 0.5) / wp) - 1.0;
            for (int k = 0; k < 16; ++k) {
                const double ah = two_pi * ch / per[k], aw = two_pi * cw / per[k];
                row[k] = (float)cos(ah);
                row[16 + k] = (float)cos(aw);
                row[32 + k] = (float)sin(ah);
                row[48 + k] = (float)sin(aw);
            }
        }
    if (hipStreamSynchronize(st) != hipSuccess ||
        hipMemcpy(table, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        gp_set_error("dino_rope_table: copy to the device failed");
        return GP_ERR_LAUNCH;
    }
    return GP_OK;
}

extern "C" int gp_dino_forward(const gp_dino_weights* wt, const float* rgb, int b, int h, int w, int n_out,
                               const int* out_layers, float* const* outs, int arith, void* workspace,
                               size_t workspace_bytes, hipStream_t st) {
    GP_REQUIRE(wt && rgb && out_layers && outs && workspace, "dino_forward: null pointer");
    GP_REQUIRE(b >= 1, "dino_forward: b=%d must be at least 1", b);
    GP_REQUIRE(h >= DN_PATCH && w >= DN_PATCH && h % DN_PATCH == 0 && w % DN_PATCH == 0,
               "dino_forward: image %d x %d must be multiples of the patch size 16", h, w);
    const int hp = h / DN_PATCH, wp = w / DN_PATCH;
    GP_REQUIRE((long long)hp * wp <= DN_MAX_PATCHES, "dino_forward: %d x %d patches exceed %d", hp, wp, DN_MAX_PATCHES);
    GP_REQUIRE(arith == GP_DINO_SPLIT_F16 || arith == GP_DINO_F32, "dino_forward: arith %d", arith);
    GP_REQUIRE(n_out >= 1 && n_out <= DN_BLOCKS, "dino_forward: n_out=%d (1..12)", n_out);
    int nblk = 0;
    for (int i = 0; i < n_out; ++i) {
        GP_REQUIRE(out_layers[i] >= 0 && out_layers[i] < DN_BLOCKS, "dino_forward: layer %d (0..11)", out_layers[i]);
        GP_REQUIRE(outs[i] && (uintptr_t)outs[i] % 16 == 0, "dino_forward: output %d is null or not 16-byte aligned", i);
        nblk = std::max(nblk, out_layers[i] + 1);
    }
    GP_REQUIRE(wt->patch_w && wt->patch_b && wt->cls_token && wt->storage_tokens && wt->norm_w && wt->norm_b && wt->rope,
               "dino_forward: null weight pointer");
    GP_REQUIRE(wt->rope_hp == hp && wt->rope_wp == wp, "dino_forward: the RoPE table is for %d x %d patches, the image has %d x %d",
               wt->rope_hp, wt->rope_wp, hp, wp);
    const bool split = arith == GP_DINO_SPLIT_F16;
    for (int l = 0; l < nblk; ++l) {
        const gp_dino_block& k = wt->blocks[l];
        GP_REQUIRE(k.ln1_w && k.ln1_b && k.ln2_w && k.ln2_b && k.qkv_b && k.proj_b && k.w12_b && k.w3_b,
                   "dino_forward: block %d has a null norm or bias pointer", l);
        GP_REQUIRE(split ? (k.qkv_h && k.proj_h && k.w12_h && k.w3_h) : (k.qkv_w && k.proj_w && k.w12_w && k.w3_w),
                   "dino_forward: block %d lacks the %s weights", l, split ? "split-f16" : "fp32");
    }
    GP_REQUIRE(((uintptr_t)rgb | (uintptr_t)workspace) % 16 == 0, "dino_forward: pointers must be 16-byte aligned");
    const int np = hp * wp, n = np + DN_PREFIX;
    int chunk = dino_chunk_cap(b, n);
    while (chunk >= 1 && sizeof(float) * dino_layout(chunk, n).total > workspace_bytes) --chunk;
    GP_REQUIRE(chunk >= 1, "dino_forward: workspace of %zu bytes, one image needs %zu", workspace_bytes,
               sizeof(float) * dino_layout(1, n).total);
    const DinoLayout L = dino_layout(chunk, n);
    float* ws = static_cast<float*>(workspace);
    float *hbuf = ws + L.h, *y = ws + L.y, *qkv = ws + L.qkv, *att = ws + L.att, *rbuf = ws + L.r, *g = ws + L.g,
          *u = ws + L.u;
    const size_t mxs = dn_align((size_t)chunk * n);
    float *ymx = ws + L.mx, *amx = ymx + mxs, *gmx = amx + mxs;
    const int nqb = (n + 63) / 64;

    for (int b0 = 0; b0 < b; b0 += chunk) {
        const int cb = std::min(chunk, b - b0), m = cb * n;
        const float* x = rgb + (size_t)b0 * 3 * h * w;
        hipLaunchKernelGGL(dino_prefix_kernel, dim3((cb * DN_PREFIX * DN_D / 4 + DN_THREADS - 1) / DN_THREADS),
                           dim3(DN_THREADS), 0, st, wt->cls_token, wt->storage_tokens, cb, n, hbuf);
        GP_TRY(gp_check_launch("dino_prefix_kernel"));
        hipLaunchKernelGGL(dino_patch_embed_kernel, dim3((cb * np + 63) / 64, DN_D / 128), dim3(DN_THREADS), 0, st, x, cb,
                           h, w, wt->patch_w, wt->patch_b, hbuf);
        GP_TRY(gp_check_launch("dino_patch_embed_kernel"));
        const float* pending = nullptr;   // fp32 path: a linear's output not yet added to h
        auto add_ln = [&](const float* gamma, const float* beta, float* dst, float* dmax, int drop) {
            hipLaunchKernelGGL(dino_add_ln_kernel, dim3((m + 3) / 4), dim3(DN_THREADS), 0, st, hbuf, pending, m, gamma,
                               beta, dst, dmax, n, drop);
            pending = nullptr;
            return gp_check_launch("dino_add_ln_kernel");
        };
        for (int l = 0; l < nblk; ++l) {
            const gp_dino_block& k = wt->blocks[l];
            GP_TRY(add_ln(k.ln1_w, k.ln1_b, y, split ? ymx : nullptr, 0));
            if (split)
                GP_TRY(gp_linear_split(y, DN_D, m, DN_D, k.qkv_h, k.qkv_b, 3 * DN_D, 0, qkv, 3 * DN_D, ymx,
                                       GP_LINEAR_RMAX_GIVEN, nullptr, st));
            else
                GP_TRY(gp_linear(y, DN_D, m, DN_D, k.qkv_w, k.qkv_b, 3 * DN_D, 0, qkv, 3 * DN_D, st));
            if (split && hipMemsetAsync(amx, 0, sizeof(float) * (size_t)m, st) != hipSuccess)
                return gp_check_launch("dino attention ymax memset");
            hipLaunchKernelGGL(dino_attention_kernel, dim3((unsigned)(nqb * DN_HEADS * cb)), dim3(DN_THREADS), 0, st, qkv,
                               wt->rope, n, nqb, att, split ? reinterpret_cast<unsigned*>(amx) : nullptr);
            GP_TRY(gp_check_launch("dino_attention_kernel"));
            if (split) {
                GP_TRY(gp_linear_split(att, DN_D, m, DN_D, k.proj_h, k.proj_b, DN_D, 4, hbuf, DN_D, amx,
                                       GP_LINEAR_RMAX_GIVEN, nullptr, st));
            } else {
                GP_TRY(gp_linear(att, DN_D, m, DN_D, k.proj_w, k.proj_b, DN_D, 0, rbuf, DN_D, st));
                pending = rbuf;
            }
            GP_TRY(add_ln(k.ln2_w, k.ln2_b, y, split ? ymx : nullptr, 0));
            if (split) {
                GP_TRY(gp_linear_split(y, DN_D, m, DN_D, k.w12_h, k.w12_b, 2 * DN_HID, 5, g, DN_HID, ymx,
                                       GP_LINEAR_RMAX_GIVEN, gmx, st));
                GP_TRY(gp_linear_split(g, DN_HID, m, DN_HID, k.w3_h, k.w3_b, DN_D, 4, hbuf, DN_D, gmx,
                                       GP_LINEAR_RMAX_GIVEN, nullptr, st));
            } else {
                GP_TRY(gp_linear(y, DN_D, m, DN_D, k.w12_w, k.w12_b, 2 * DN_HID, 0, u, 2 * DN_HID, st));
                const size_t total4 = (size_t)m * (DN_HID / 4);
                hipLaunchKernelGGL(dino_swiglu_kernel, dim3((unsigned)((total4 + DN_THREADS - 1) / DN_THREADS)),
                                   dim3(DN_THREADS), 0, st, u, total4, g);
                GP_TRY(gp_check_launch("dino_swiglu_kernel"));
                GP_TRY(gp_linear(g, DN_HID, m, DN_HID, k.w3_w, k.w3_b, DN_D, 0, rbuf, DN_D, st));
                pending = rbuf;
            }
            for (int i = 0; i < n_out; ++i)
                if (out_layers[i] == l)
                    GP_TRY(add_ln(wt->norm_w, wt->norm_b, outs[i] + (size_t)b0 * np * DN_D, nullptr, DN_PREFIX));
        }
    }
    return GP_OK;
}
