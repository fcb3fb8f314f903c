// RGB-D front end for gfx950: one depth / colour / instance-mask frame -> the per-object batch the pose
// networks read (DESIGN.md "RGB-D front end"; the meaning of datasets/datasets_infer.py InferDataset).
//
//   frame_mask_stats_kernel   one pass over the mask -> per id {count, rmin, rmax, cmin, cmax}
//   gp_frame_crop_boxes       HOST: ids present (ascending, 255 = background) and their crop boxes
//   frame_objects_kernel      one workgroup per object: compaction of the crop's valid pixels, the sample of
//                             n_pts of them (tiling, or a keyed random selection), back-projection
//   frame_roi_rgb_kernel      bilinear colour crop, uint8 rounding, ImageNet normalisation, CHW
//
// The gp_frames_* entries take F frames of one size stacked contiguously and the objects of all of them in one
// launch: the statistics kernels carry the frame as a grid dimension, frames_objects_kernel and
// frames_roi_rgb_kernel run the single-frame bodies on frame frame_of[b].
//
// Everything is integer or separately rounded fp32 / fp64 arithmetic with a fixed order, and the only atomics
// are integer ones whose result does not depend on their order, so every output is bitwise reproducible.
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "gp_common.h"

#define FR_IDS 256          // mask values
#define FR_BACKGROUND 255
#define FR_STAT 5           // count, rmin, rmax, cmin, cmax
#define FR_SEG 16           // pixels of one row a thread of the statistics pass walks
#define FR_THREADS 1024     // frame_objects_kernel workgroup
#define FR_WAVES (FR_THREADS / GP_WAVE)
#define FR_MAX_PTS 2048
#define FR_SAMPLE_TAG 0x53414D50u   // "SAMP": the sampling keys' Philox counter word 3
#define FR_MAX_FRAMES 65535 // frames of one gp_frames_* call (a grid dimension of the statistics pass)

// ============================================================================ mask statistics
// blockIdx.x is the frame (one frame: a grid of 1)
__global__ __launch_bounds__(FR_IDS) void frame_stats_init_kernel(int* __restrict__ stats, int h, int w) {
    const int id = threadIdx.x;
    stats += (size_t)blockIdx.x * FR_IDS * FR_STAT;
    stats[id * FR_STAT + 0] = 0;
    stats[id * FR_STAT + 1] = h;
    stats[id * FR_STAT + 2] = -1;
    stats[id * FR_STAT + 3] = w;
    stats[id * FR_STAT + 4] = -1;
}

// A run of equal ids inside one row segment: one LDS update per run, not per pixel (the background is most
// of a frame).
__device__ __forceinline__ void stats_flush(int* s_tab, int id, int cnt, int r, int c0, int c1) {
    int* t = s_tab + id * FR_STAT;
    atomicAdd(t + 0, cnt);
    atomicMin(t + 1, r);
    atomicMax(t + 2, r);
    atomicMin(t + 3, c0);
    atomicMax(t + 4, c1);
}

__global__ __launch_bounds__(256) void frame_mask_stats_kernel(const uint8_t* __restrict__ mask, int h, int w,
                                                                int segs_per_row, int* __restrict__ stats) {
    __shared__ int s_tab[FR_IDS * FR_STAT];
    mask += (size_t)blockIdx.y * h * w;   // blockIdx.y is the frame (one frame: gridDim.y = 1)
    stats += (size_t)blockIdx.y * FR_IDS * FR_STAT;
    for (int id = threadIdx.x; id < FR_IDS; id += blockDim.x) {
        s_tab[id * FR_STAT + 0] = 0;
        s_tab[id * FR_STAT + 1] = h;
        s_tab[id * FR_STAT + 2] = -1;
        s_tab[id * FR_STAT + 3] = w;
        s_tab[id * FR_STAT + 4] = -1;
    }
    __syncthreads();
    const long long nseg = (long long)h * segs_per_row;
    for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < nseg;
         s += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(s / segs_per_row);
        const int c0 = (int)(s % segs_per_row) * FR_SEG;
        const int c1 = min(c0 + FR_SEG, w);
        const uint8_t* row = mask + (size_t)r * w;
        int id = row[c0], start = c0;
        for (int c = c0 + 1; c < c1; ++c) {
            const int v = row[c];
            if (v != id) {
                stats_flush(s_tab, id, c - start, r, start, c - 1);
                id = v;
                start = c;
            }
        }
        stats_flush(s_tab, id, c1 - start, r, start, c1 - 1);
    }
    __syncthreads();
    // one integer atomic per (workgroup, id present, field)
    for (int id = threadIdx.x; id < FR_IDS; id += blockDim.x) {
        const int* t = s_tab + id * FR_STAT;
        if (t[0] > 0) {
            int* g = stats + id * FR_STAT;
            atomicAdd(g + 0, t[0]);
            atomicMin(g + 1, t[1]);
            atomicMax(g + 2, t[2]);
            atomicMin(g + 3, t[3]);
            atomicMax(g + 4, t[4]);
        }
    }
}

// the init launch and the statistics launch over f frames
static int launch_mask_stats(const uint8_t* mask, int f, int h, int w, int* stats, hipStream_t stream) {
    hipLaunchKernelGGL(frame_stats_init_kernel, dim3(f), dim3(FR_IDS), 0, stream, stats, h, w);
    const int segs = (w + FR_SEG - 1) / FR_SEG;
    const long long nseg = (long long)h * segs;
    const int blocks = (int)std::min<long long>((nseg + 255) / 256, 256);
    hipLaunchKernelGGL(frame_mask_stats_kernel, dim3(blocks, f), dim3(256), 0, stream, mask, h, w, segs, stats);
    return gp_check_launch("frame_mask_stats_kernel");
}

extern "C" int gp_frame_mask_stats(const uint8_t* mask, int h, int w, int* stats, hipStream_t stream) {
    GP_REQUIRE(mask && stats, "frame_mask_stats: null pointer");
    GP_REQUIRE(h >= 1 && w >= 1 && (long long)h * w < INT_MAX, "frame_mask_stats: bad frame size %d x %d", h, w);
    return launch_mask_stats(mask, 1, h, w, stats, stream);
}

extern "C" int gp_frames_mask_stats(const uint8_t* mask, int f, int h, int w, int* stats, hipStream_t stream) {
    GP_REQUIRE(mask && stats, "frames_mask_stats: null pointer");
    GP_REQUIRE(f >= 1 && f <= FR_MAX_FRAMES, "frames_mask_stats: f=%d (1..%d)", f, FR_MAX_FRAMES);
    GP_REQUIRE(h >= 1 && w >= 1 && (long long)h * w < INT_MAX, "frames_mask_stats: bad frame size %d x %d", h, w);
    return launch_mask_stats(mask, f, h, w, stats, stream);
}

// ============================================================================ crop boxes (host)
// The square crop window of utils/sgpa_utils.py get_bbox (40-pixel multiples, at most h-40 / w-40, shifted back
// inside the image) and the centre / scale of utils/datasets_utils.py aug_bbox_eval, in integer arithmetic.
extern "C" int gp_frame_crop_boxes(const int* stats_host, int h, int w, int* ids_out, float* boxes_out,
                                   int* n_out) {
    GP_REQUIRE(stats_host && ids_out && boxes_out && n_out, "frame_crop_boxes: null pointer");
    GP_REQUIRE(h > 40 && w > 40, "frame_crop_boxes: the frame must be larger than 40 x 40 (got %d x %d)", h, w);
    int n = 0;
    for (int id = 0; id < FR_IDS; ++id) {
        if (id == FR_BACKGROUND) continue;
        const int* t = stats_host + id * FR_STAT;
        if (t[0] <= 0) continue;
        const int y1 = t[1], y2 = t[2], x1 = t[3], x2 = t[4];
        GP_REQUIRE(y1 >= 0 && y1 <= y2 && y2 < h && x1 >= 0 && x1 <= x2 && x2 < w,
                   "frame_crop_boxes: id %d has the box rows [%d, %d], columns [%d, %d] outside %d x %d", id, y1, y2,
                   x1, x2, h, w);
        int win = (std::max(y2 - y1, x2 - x1) / 40 + 1) * 40;
        win = std::min(win, std::min(h - 40, w - 40));
        const int half = win / 2;
        const int cr = (y1 + y2) / 2, cc = (x1 + x2) / 2;
        int rmin = cr - half, rmax = cr + half, cmin = cc - half, cmax = cc + half;
        if (rmin < 0) { rmax -= rmin; rmin = 0; }
        if (cmin < 0) { cmax -= cmin; cmin = 0; }
        if (rmax > h) { rmin -= rmax - h; rmax = h; }
        if (cmax > w) { cmin -= cmax - w; cmax = w; }
        ids_out[n] = id;
        boxes_out[3 * n + 0] = 0.5f * (float)(cmin + cmax);
        boxes_out[3 * n + 1] = 0.5f * (float)(rmin + rmax);
        boxes_out[3 * n + 2] = (float)std::min(std::max(rmax - rmin, cmax - cmin), std::max(h, w));
        ++n;
    }
    *n_out = n;
    return GP_OK;
}

// ============================================================================ crop mapping
// Crop pixel (i, j) of the S x S crop reads the source position (u, v) = ((j - S/2) scale / S + cx,
// (i - S/2) scale / S + cy) in double: the inverse of the reference's affine transform without rotation.
__device__ __forceinline__ double crop_src(int k, int s, float scale, float centre) {
#pragma clang fp contract(off)
    return (double)(k - s / 2) * (double)scale / (double)s + (double)centre;
}
// nearest source index, or -1 outside [0, n)
__device__ __forceinline__ int crop_nearest(int k, int s, float scale, float centre, int n) {
#pragma clang fp contract(off)
    const double f = floor(crop_src(k, s, scale, centre) + 0.5);
    return (f >= 0.0 && f < (double)n) ? (int)f : -1;
}

// ============================================================================ objects
// The 64-bit sort item of element e (its position in V): Philox word 0 above e. Items are distinct, so the
// n_pts smallest are a unique set and (key, e) ascending a unique order.
__device__ __forceinline__ uint64_t sample_item(uint32_t e, uint32_t id, uint32_t k0, uint32_t k1) {
    const u32x4 r = philox4x32_10(u32x4{e, id, 0u, FR_SAMPLE_TAG}, k0, k1);
    return ((uint64_t)r.x << 32) | e;
}

// Object b without a valid pixel (the caller raises on count < 10): defined outputs all the same.
__device__ __forceinline__ void object_zero_outputs(int b, int n_pts, float* __restrict__ pts,
                                                    int* __restrict__ roi_xs, int* __restrict__ roi_ys) {
    float* opts = pts + (size_t)b * n_pts * 3;
    int* oxs = roi_xs + (size_t)b * n_pts;
    int* oys = roi_ys + (size_t)b * n_pts;
    for (int j = threadIdx.x; j < n_pts; j += FR_THREADS) {
        opts[3 * j] = opts[3 * j + 1] = opts[3 * j + 2] = 0.f;
        oxs[j] = oys[j] = 0;
    }
}

// Object b = blockIdx.x of the (h,w) frame at depth / mask, camera {fx, fy, cx, cy}, sampling key {k0, k1}: the
// body of frame_objects_kernel (one frame) and frames_objects_kernel (the frame of frame_of[b]).
__device__ __forceinline__ void frame_objects_body(
    const float* __restrict__ depth, const uint8_t* __restrict__ mask, int h, int w, const int* __restrict__ ids,
    const float* __restrict__ boxes, int s, int n_pts, int n_sort, float fx, float fy, float cx, float cy,
    float max_depth, uint32_t k0, uint32_t k1, uint32_t* __restrict__ vws, float* __restrict__ pts,
    int* __restrict__ roi_xs, int* __restrict__ roi_ys, int* __restrict__ count) {
    __shared__ int s_wcnt[FR_WAVES];
    __shared__ unsigned s_hist[256];
    __shared__ unsigned long long s_prefix;
    __shared__ unsigned s_rank, s_fill;
    __shared__ unsigned long long s_items[FR_MAX_PTS];

    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (GP_WAVE - 1), wave = tid / GP_WAVE;
    const int id = ids[b];
    const float bcx = boxes[3 * b + 0], bcy = boxes[3 * b + 1], bsc = boxes[3 * b + 2];
    const int npix = s * s;
    uint32_t* V = vws + (size_t)b * npix;

    // ---- compaction: V = the crop's valid pixels in row-major order (ballot ranks inside a wave, an in-order
    // scan of the wave totals, chunk after chunk)
    int base = 0;
    for (int p0 = 0; p0 < npix; p0 += FR_THREADS) {
        const int p = p0 + tid;
        bool valid = false;
        if (p < npix) {
            const int row = crop_nearest(p / s, s, bsc, bcy, h);
            const int col = crop_nearest(p % s, s, bsc, bcx, w);
            if (row >= 0 && col >= 0) {
                const size_t q = (size_t)row * w + col;
                const float d = depth[q];
                valid = mask[q] == id && d > 0.f && d <= max_depth;
            }
        }
        const uint64_t bal = __ballot(valid);
        if (lane == 0) s_wcnt[wave] = __popcll(bal);
        __syncthreads();
        int woff = 0, total = 0;
#pragma unroll
        for (int k = 0; k < FR_WAVES; ++k) {
            const int c = s_wcnt[k];
            woff += k < wave ? c : 0;
            total += c;
        }
        if (valid) {
            const int e = base + woff + __popcll(bal & ((1ull << lane) - 1ull));
            if (e < npix) V[e] = (uint32_t)p;
        }
        base += total;
        __syncthreads();
    }
    const int c = base;   // <= npix
    if (tid == 0) count[b] = c;

    // ---- which element each output slot takes
    float* opts = pts + (size_t)b * n_pts * 3;
    int* oxs = roi_xs + (size_t)b * n_pts;
    int* oys = roi_ys + (size_t)b * n_pts;
    if (c == 0) {   // nothing to sample
        object_zero_outputs(b, n_pts, pts, roi_xs, roi_ys);
        return;
    }
    const bool select = c >= n_pts;
    if (select) {
        // radix select of the item of rank n_pts - 1 among the c items, one byte per pass from the top; the
        // bytes of e above c's width are zero for every item and are skipped
        if (tid == 0) {
            s_prefix = 0ull;
            s_rank = (unsigned)(n_pts - 1);
        }
        for (int byte = 7; byte >= 0; --byte) {
            const int shift = 8 * byte;
            if (byte < 4 && ((uint32_t)(c - 1) >> shift) == 0u) {
                __syncthreads();
                if (tid == 0) s_prefix <<= 8;
                continue;
            }
            if (tid < 256) s_hist[tid] = 0u;
            __syncthreads();
            const uint64_t prefix = s_prefix;
            for (int e = tid; e < c; e += FR_THREADS) {
                const uint64_t it = sample_item((uint32_t)e, (uint32_t)id, k0, k1);
                if (byte == 7 || (it >> (shift + 8)) == prefix) atomicAdd(&s_hist[(it >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned r = s_rank, bin = 0;
                for (; bin < 255u && r >= s_hist[bin]; ++bin) r -= s_hist[bin];
                s_rank = r;
                s_prefix = (prefix << 8) | bin;
            }
            __syncthreads();   // the histogram is read to the end before the next pass clears it
        }
        __syncthreads();
        const uint64_t thr = s_prefix;   // the n_pts-th smallest item
        for (int j = tid; j < n_sort; j += FR_THREADS) s_items[j] = ~0ull;
        if (tid == 0) s_fill = 0u;
        __syncthreads();
        for (int e = tid; e < c; e += FR_THREADS) {
            const uint64_t it = sample_item((uint32_t)e, (uint32_t)id, k0, k1);
            if (it <= thr) {
                const unsigned slot = atomicAdd(&s_fill, 1u);
                if (slot < (unsigned)n_pts) s_items[slot] = it;
            }
        }
        __syncthreads();
        // bitonic sort of n_sort (a power of two >= n_pts, <= 2048) items; the padding sorts last
        for (int k = 2; k <= n_sort; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < n_sort; i += FR_THREADS) {
                    const int l = i ^ j;
                    if (l > i) {
                        const uint64_t a = s_items[i], z = s_items[l];
                        if (((i & k) == 0) == (a > z)) {
                            s_items[i] = z;
                            s_items[l] = a;
                        }
                    }
                }
                __syncthreads();
            }
        }
    }

    // ---- outputs: crop row / column and the back-projected point, each fp32 operation rounded on its own
    for (int j = tid; j < n_pts; j += FR_THREADS) {
        uint32_t e = select ? (uint32_t)s_items[j] : (uint32_t)(j % c);
        if (e >= (uint32_t)c) e = 0u;
        const int p = (int)V[e];
        const int ci = p / s, cj = p % s;
        const int row = crop_nearest(ci, s, bsc, bcy, h);
        const int col = crop_nearest(cj, s, bsc, bcx, w);
        float d = 0.f;
        if (row >= 0 && col >= 0) d = depth[(size_t)row * w + col];
        opts[3 * j + 0] = fdiv(fmul(fsub((float)col, cx), d), fx);
        opts[3 * j + 1] = fdiv(fmul(fsub((float)row, cy), d), fy);
        opts[3 * j + 2] = d;
        oxs[j] = ci;
        oys[j] = cj;
    }
}

__global__ __launch_bounds__(FR_THREADS) void frame_objects_kernel(
    const float* __restrict__ depth, const uint8_t* __restrict__ mask, int h, int w, const int* __restrict__ ids,
    const float* __restrict__ boxes, int s, int n_pts, int n_sort, float fx, float fy, float cx, float cy,
    float max_depth, uint32_t k0, uint32_t k1, uint32_t* __restrict__ vws, float* __restrict__ pts,
    int* __restrict__ roi_xs, int* __restrict__ roi_ys, int* __restrict__ count) {
    frame_objects_body(depth, mask, h, w, ids, boxes, s, n_pts, n_sort, fx, fy, cx, cy, max_depth, k0, k1, vws, pts,
                       roi_xs, roi_ys, count);
}

// F stacked frames: object b reads frame frame_of[b], that frame's camera intr[4 f ..] and key seeds[2 f ..]. A
// frame index outside [0, F) reads nothing: count 0 and zeroed outputs.
__global__ __launch_bounds__(FR_THREADS) void frames_objects_kernel(
    const float* __restrict__ depth, const uint8_t* __restrict__ mask, int nf, int h, int w,
    const int* __restrict__ frame_of, const int* __restrict__ ids, const float* __restrict__ boxes, int s, int n_pts,
    int n_sort, const float* __restrict__ intr, float max_depth, const uint32_t* __restrict__ seeds,
    uint32_t* __restrict__ vws, float* __restrict__ pts, int* __restrict__ roi_xs, int* __restrict__ roi_ys,
    int* __restrict__ count) {
    const int b = blockIdx.x;
    const int f = frame_of[b];
    if (f < 0 || f >= nf) {   // the same for the whole workgroup
        if (threadIdx.x == 0) count[b] = 0;
        object_zero_outputs(b, n_pts, pts, roi_xs, roi_ys);
        return;
    }
    const size_t off = (size_t)f * h * w;
    frame_objects_body(depth + off, mask + off, h, w, ids, boxes, s, n_pts, n_sort, intr[4 * f + 0], intr[4 * f + 1],
                       intr[4 * f + 2], intr[4 * f + 3], max_depth, seeds[2 * f + 0], seeds[2 * f + 1], vws, pts,
                       roi_xs, roi_ys, count);
}

extern "C" size_t gp_frame_objects_workspace_size(int b, int img_size) {
    if (b <= 0 || img_size <= 0) return 0;
    return (size_t)b * img_size * img_size * sizeof(uint32_t);
}

static int frame_check_common(const char* what, int h, int w, int b, int img_size) {
    GP_REQUIRE(b >= 0, "%s: b=%d", what, b);
    GP_REQUIRE(h >= 1 && w >= 1 && (long long)h * w < INT_MAX, "%s: bad frame size %d x %d", what, h, w);
    GP_REQUIRE(img_size >= 14 && img_size <= 4096 && img_size % 2 == 0,
               "%s: img_size=%d (an even size in [14, 4096])", what, img_size);
    return GP_OK;
}

extern "C" int gp_frame_objects(const float* depth, const uint8_t* mask, int h, int w, const int* ids,
                                const float* boxes, int b, int img_size, int n_pts, float fx, float fy, float cx,
                                float cy, float max_depth, uint64_t seed, float* pts, int* roi_xs, int* roi_ys,
                                int* count, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (int rc = frame_check_common("frame_objects", h, w, b, img_size)) return rc;
    GP_REQUIRE(n_pts >= 1 && n_pts <= FR_MAX_PTS, "frame_objects: n_pts=%d (1..%d)", n_pts, FR_MAX_PTS);
    GP_REQUIRE(pts && roi_xs && roi_ys && count, "frame_objects: null output");
    if (b == 0) return GP_OK;
    GP_REQUIRE(depth && mask && ids && boxes, "frame_objects: null input");
    GP_REQUIRE(fx != 0.f && fy != 0.f, "frame_objects: zero focal length");
    GP_REQUIRE(workspace && workspace_bytes >= gp_frame_objects_workspace_size(b, img_size),
               "frame_objects: workspace of %zu bytes, %zu needed", workspace_bytes,
               gp_frame_objects_workspace_size(b, img_size));
    int n_sort = 2;
    while (n_sort < n_pts) n_sort <<= 1;
    hipLaunchKernelGGL(frame_objects_kernel, dim3(b), dim3(FR_THREADS), 0, stream, depth, mask, h, w, ids, boxes,
                       img_size, n_pts, n_sort, fx, fy, cx, cy, max_depth, (uint32_t)seed, (uint32_t)(seed >> 32),
                       static_cast<uint32_t*>(workspace), pts, roi_xs, roi_ys, count);
    return gp_check_launch("frame_objects_kernel");
}

extern "C" int gp_frames_objects(const float* depth, const uint8_t* mask, int f, int h, int w, const int* frame_of,
                                 const int* ids, const float* boxes, int b, int img_size, int n_pts,
                                 const float* intr, float max_depth, const uint32_t* seeds, float* pts, int* roi_xs,
                                 int* roi_ys, int* count, void* workspace, size_t workspace_bytes,
                                 hipStream_t stream) {
    GP_REQUIRE(f >= 1 && f <= FR_MAX_FRAMES, "frames_objects: f=%d (1..%d)", f, FR_MAX_FRAMES);
    if (int rc = frame_check_common("frames_objects", h, w, b, img_size)) return rc;
    GP_REQUIRE(b <= 65535, "frames_objects: b=%d exceeds 65535", b);
    GP_REQUIRE(n_pts >= 1 && n_pts <= FR_MAX_PTS, "frames_objects: n_pts=%d (1..%d)", n_pts, FR_MAX_PTS);
    GP_REQUIRE(pts && roi_xs && roi_ys && count, "frames_objects: null output");
    if (b == 0) return GP_OK;
    GP_REQUIRE(depth && mask && frame_of && ids && boxes && intr && seeds, "frames_objects: null input");
    GP_REQUIRE(workspace && workspace_bytes >= gp_frame_objects_workspace_size(b, img_size),
               "frames_objects: workspace of %zu bytes, %zu needed", workspace_bytes,
               gp_frame_objects_workspace_size(b, img_size));
    int n_sort = 2;
    while (n_sort < n_pts) n_sort <<= 1;
    hipLaunchKernelGGL(frames_objects_kernel, dim3(b), dim3(FR_THREADS), 0, stream, depth, mask, f, h, w, frame_of, ids,
                       boxes, img_size, n_pts, n_sort, intr, max_depth, seeds, static_cast<uint32_t*>(workspace), pts,
                       roi_xs, roi_ys, count);
    return gp_check_launch("frames_objects_kernel");
}

// ============================================================================ colour crop
// One thread per crop pixel: bilinear taps of the uint8 colour image at (u, v) (taps outside the image are 0),
// rounded to a uint8 level as floor(value + 0.5), then (level / 255 - mean) / std, stored channel-major.
// The body of frame_roi_rgb_kernel (one frame) and frames_roi_rgb_kernel (the frame of frame_of[b]).
__device__ __forceinline__ void frame_roi_rgb_body(const uint8_t* __restrict__ color, int h, int w,
                                                   const float* __restrict__ boxes, int s, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int npix = s * s;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const float bcx = boxes[3 * b + 0], bcy = boxes[3 * b + 1], bsc = boxes[3 * b + 2];
    const double u = crop_src(p % s, s, bsc, bcx), v = crop_src(p / s, s, bsc, bcy);
    const double fu = floor(u), fv = floor(v);
    const double ax = u - fu, ay = v - fv;
    // taps further than one pixel outside contribute nothing: clamp before the integer conversion
    const int x0 = (int)fmin(fmax(fu, -2.0), (double)w), y0 = (int)fmin(fmax(fv, -2.0), (double)h);
    const double mean[3] = {0.485, 0.456, 0.406}, sd[3] = {0.229, 0.224, 0.225};
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int x = x0 + (t & 1), y = y0 + (t >> 1);
        const double wt = ((t & 1) ? ax : 1.0 - ax) * ((t >> 1) ? ay : 1.0 - ay);
        if (x >= 0 && x < w && y >= 0 && y < h) {
            const uint8_t* px = color + ((size_t)y * w + x) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) acc[ch] += wt * (double)px[ch];
        }
    }
    float* o = out + (size_t)b * 3 * npix + p;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double q = fmin(fmax(floor(acc[ch] + 0.5), 0.0), 255.0);
        o[(size_t)ch * npix] = (float)((q / 255.0 - mean[ch]) / sd[ch]);
    }
}

__global__ __launch_bounds__(256) void frame_roi_rgb_kernel(const uint8_t* __restrict__ color, int h, int w,
                                                             const float* __restrict__ boxes, int s,
                                                             float* __restrict__ out) {
    frame_roi_rgb_body(color, h, w, boxes, s, out);
}

// A frame index outside [0, F) is an image of no pixels: every tap lies outside, nothing is read, level 0.
__global__ __launch_bounds__(256) void frames_roi_rgb_kernel(const uint8_t* __restrict__ color, int nf, int h, int w,
                                                              const int* __restrict__ frame_of,
                                                              const float* __restrict__ boxes, int s,
                                                              float* __restrict__ out) {
    const int f = frame_of[blockIdx.y];
    if (f < 0 || f >= nf) {
        frame_roi_rgb_body(color, 0, 0, boxes, s, out);
        return;
    }
    frame_roi_rgb_body(color + (size_t)f * h * w * 3, h, w, boxes, s, out);
}

extern "C" int gp_frame_roi_rgb(const uint8_t* color, int h, int w, const float* boxes, int b, int img_size,
                                float* roi_rgb, hipStream_t stream) {
    if (int rc = frame_check_common("frame_roi_rgb", h, w, b, img_size)) return rc;
    GP_REQUIRE(roi_rgb, "frame_roi_rgb: null output");
    if (b == 0) return GP_OK;
    GP_REQUIRE(color && boxes, "frame_roi_rgb: null input");
    GP_REQUIRE(b <= 65535, "frame_roi_rgb: b=%d exceeds 65535", b);
    const int npix = img_size * img_size;
    hipLaunchKernelGGL(frame_roi_rgb_kernel, dim3((npix + 255) / 256, b), dim3(256), 0, stream, color, h, w, boxes,
                       img_size, roi_rgb);
    return gp_check_launch("frame_roi_rgb_kernel");
}

extern "C" int gp_frames_roi_rgb(const uint8_t* color, int f, int h, int w, const int* frame_of, const float* boxes,
                                 int b, int img_size, float* roi_rgb, hipStream_t stream) {
    GP_REQUIRE(f >= 1 && f <= FR_MAX_FRAMES, "frames_roi_rgb: f=%d (1..%d)", f, FR_MAX_FRAMES);
    if (int rc = frame_check_common("frames_roi_rgb", h, w, b, img_size)) return rc;
    GP_REQUIRE(b <= 65535, "frames_roi_rgb: b=%d exceeds 65535", b);
    GP_REQUIRE(roi_rgb, "frames_roi_rgb: null output");
    if (b == 0) return GP_OK;
    GP_REQUIRE(color && frame_of && boxes, "frames_roi_rgb: null input");
    const int npix = img_size * img_size;
    hipLaunchKernelGGL(frames_roi_rgb_kernel, dim3((npix + 255) / 256, b), dim3(256), 0, stream, color, f, h, w,
                       frame_of, boxes, img_size, roi_rgb);
    return gp_check_launch("frames_roi_rgb_kernel");
}
