// Data step of one KITTI SEQUENCE item on the device (reference datasets/kitti_dataset_seq.py:100-175 `__getitem__` /
// `get_color`): n + 2 consecutive frames, read as three windows of n frames (centre 1..n, left 0..n-1, right 2..n+1).
// Per frame and per level s the reference runs
//     r = Lanczos resize of u[s-1];  m = mirror(r) if do_flip;  u[s] = ColorJitter_fresh(m) if do_color_aug;  color = u[s] / 255
// so the mirror accumulates from level to level and level s + 1 is resized from the JITTERED level s.
//   * without jitter the three windows are overlapping slices of one (n + 2)-frame pyramid: n + 2 images are made, none twice;
//   * with jitter every (window, frame, level) has its own draw: 3n images, image i = w * n + j gathers frame j + (1, 0, 2)[w].
// A STEP may hold several items (dc_data_seq_batch_levels): their images are stacked time-major -- image t * items + item, t the
// frame or the window slot -- so that one time step of all items is a contiguous slab; the frames arrive item-major, each item
// has its own mirror flag and jitter rows, and the launches are those of one item (seq_item / seq_src / seq_jrow / seq_flip).
// Two ways through a level, the same bytes either way (tests/test_seq_data_gpu.py runs every split):
//   * through HBM, the whole machine on every level: the two dc_data_resize_axis passes, an integer luma-sum pass when
//     jittered, and one finish pass (mirror, jitter, uint8 + float stores) over all images at once;
//   * tail kernel: one workgroup per image carries it from the first level whose uint8 form fits the LDS budget down to
//     the last, entirely on chip -- both resize passes, the mirror, the jitter (block-wide integer reduction for the
//     contrast mean) and the float stores of every level, in ONE launch.
// A tail puts one compute unit on an image, so its time grows with the image while a launch over all images stays at its
// fixed cost: measured at 192 x 640 (tools/time_seq_loader.py --lds_budget) a tail from level 1 takes 0.60 ms
// per item where the HBM levels take 0.15 ms, and it still loses from level 3.  The default budget therefore hands the
// tail only levels of a few KB (small training sizes, where it does save launches); a caller may raise it up to the
// hardware's 160 KiB per workgroup.
// The arithmetic is data_dev.h's, shared with data.hip.  Sums are integers throughout: two calls give the same bits.
#include "data_dev.h"

#include <algorithm>

namespace dc {

constexpr int kSeqThreads = 1024;          // tail kernel: 16 waves on one CU
constexpr int kSeqStripRows = 8;           // output rows per strip of the tail's first resize (its source is in HBM)
constexpr int kSeqKsize = 13;              // dc_resample_ksize(2 m, m): every level halves the one before
constexpr int kSeqStripSrcRows = 2 * kSeqStripRows + 12;   // source rows one strip may span (2 R + 9 with Pillow's tables)
constexpr int kSeqLdsCap = 160 * 1024 - 256;               // gfx950: 160 KiB per workgroup, less the static reduction words
constexpr int kSeqMaxItems = 64;                          // sequence items per step (their flip flags travel as kernel arguments)
constexpr int kSeqLdsDefault = 12 * 1024;                  // the tail's default budget: below the smallest level of 192 x 640 (see above)

struct SeqTabs {   // device tables of level s (1..S-1): (size >> (s - 1)) -> (size >> s) along each axis
    const int* bx[DC_MAX_SCALES];
    const int* kx[DC_MAX_SCALES];
    const int* by[DC_MAX_SCALES];
    const int* ky[DC_MAX_SCALES];
};
struct SeqArgs {
    const uint8_t* src;            // tail / finish input: level-0 frames (gathered) or the images of the level before
    uint8_t* u8;                   // finish: u[s] (n_img, h, w, 3), or NULL when no level follows
    float* color[DC_MAX_SCALES];
    float4* packed;
    const int* steps;              // (n_img, S, 4) or NULL
    const float* params;
    unsigned long long* sums;      // (n_img, S): the tiled levels' luma sums
    int n, S, H, W;
    int items;                     // sequence items of the step: image i is frame / window slot i / items of item i % items (time-major)
    unsigned flips[kSeqMaxItems / 32];   // one bit per item
    int gather;                    // the launch reads level 0: image i comes from frame seq_src(a, i) of `src` (item-major, unmirrored)
    int level;                     // finish: the level; tail: its first level
    int b_off;                     // tail: byte offset of the second LDS buffer
    SeqTabs tabs;
};

__device__ __forceinline__ int seq_frame(int i, int n) {
    const int w = i / n, j = i - w * n;
    return j + (w == 0 ? 1 : (w == 1 ? 0 : 2));   // windows in the order centre, left, right
}
// The image index of a step of `items` sequence items is time-major: im = t * items + item, t = the frame (un-jittered,
// 0..n+1) or the window slot w * n + j (jittered, 0..3n-1).  These three say what an image reads; items == 1 gives im itself.
__device__ __forceinline__ int seq_item(const SeqArgs& a, int im) { return im % a.items; }
__device__ __forceinline__ int seq_flip(const SeqArgs& a, int im) {
    const int it = seq_item(a, im);
    return (a.flips[it >> 5] >> (it & 31)) & 1;
}
// level-0 source frame: the frames are uploaded item-major, n + 2 per item
__device__ __forceinline__ int seq_src(const SeqArgs& a, int im) {
    const int t = im / a.items;
    return seq_item(a, im) * (a.n + 2) + (a.steps ? seq_frame(t, a.n) : t);
}
// row of the jitter tables: item-major, 3n rows per item
__device__ __forceinline__ int seq_jrow(const SeqArgs& a, int im) { return seq_item(a, im) * 3 * a.n + im / a.items; }

// ---- levels that live in HBM -------------------------------------------------------------------------------------------
// exact luma sum of every image in front of its contrast step at `level` (the mirror does not change a sum)
__global__ __launch_bounds__(256) void seq_sum_kernel(const SeqArgs a) {
    const int im = blockIdx.y, s = a.level;
    const JChain ch = jchain_load(a.steps, a.params, seq_jrow(a, im) * a.S + s);
    if (ch.c < 0) return;
    const int npix = (a.H >> s) * (a.W >> s);
    const uint8_t* p = a.src + (size_t)(a.gather ? seq_src(a, im) : im) * npix * 3;
    unsigned int acc = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
        int r = p[3 * i], g = p[3 * i + 1], b = p[3 * i + 2];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < ch.c) jitter_op(r, g, b, ch.op[k], ch.a[k], 0);
        acc += luma(r, g, b);
    }
    unsigned long long v = acc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __shared__ unsigned long long part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&a.sums[(size_t)im * a.S + s], part[0] + part[1] + part[2] + part[3]);   // integer: order-free
}
// mirror, jitter, and the stores of one level: u[s] for the next level's resize, ("color", s), RGBx at level 0
__global__ __launch_bounds__(256) void seq_finish_kernel(const SeqArgs a) {
    const int im = blockIdx.y, s = a.level;
    const int w = a.W >> s, npix = (a.H >> s) * w;
    const JChain ch = jchain_load(a.steps, a.params, seq_jrow(a, im) * a.S + s);
    const int mean = ch.c >= 0 ? luma_mean(a.sums[(size_t)im * a.S + s], npix) : 0;
    const uint8_t* p = a.src + (size_t)(a.gather ? seq_src(a, im) : im) * npix * 3;
    uint8_t* u = a.u8 ? a.u8 + (size_t)im * npix * 3 : nullptr;
    float* o = a.color[s] + (size_t)im * npix * 3;
    float4* pk = (s == 0 && a.packed) ? a.packed + (size_t)im * npix : nullptr;
    const int flip = seq_flip(a, im);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
        int src = i;
        if (flip) {
            const int y = i / w;
            src = 2 * y * w + w - 1 - i;     // (y, w - 1 - x)
        }
        const uint8_t* q = p + (size_t)3 * src;
        int r = q[0], g = q[1], b = q[2];
#pragma unroll
        for (int k = 0; k < 4; ++k) jitter_op(r, g, b, ch.op[k], ch.a[k], mean);
        if (u) u[3 * i] = (uint8_t)r, u[3 * i + 1] = (uint8_t)g, u[3 * i + 2] = (uint8_t)b;
        const float fr = (float)r / 255.0f, fg = (float)g / 255.0f, fb = (float)b / 255.0f;
        o[i] = fr;
        o[(size_t)npix + i] = fg;
        o[(size_t)2 * npix + i] = fb;
        if (pk) pk[i] = make_float4(fr, fg, fb, 0.f);
    }
}

// ---- tail: one workgroup per image, levels a.level .. S-1 on chip ----------------------------------------------------------
// LDS: A = the current level's uint8 image (HWC), B = the horizontal pass's output.  Level t (the first) comes from HBM:
// t = 0 copies its frame (mirrored on the way in); t > 0 resizes u[t-1] strip by strip -- kSeqStripRows output rows need
// at most kSeqStripSrcRows source rows, made by the horizontal pass into B and consumed by the vertical pass into A, so
// that the 4x larger source never has to fit.  Every later level reads A, writes B (h_prev x w), then A again.
// Every barrier is reached by the whole block: loop bounds depend on launch constants and the block's tables only.
__global__ __launch_bounds__(kSeqThreads) void seq_tail_kernel(const SeqArgs a) {
    extern __shared__ __align__(16) uint8_t seq_lds[];
    __shared__ unsigned long long part[kSeqThreads / 64];
    uint8_t* A = seq_lds;
    uint8_t* Bf = seq_lds + a.b_off;
    const int im = blockIdx.x, tid = threadIdx.x, t = a.level;
    int h = a.H >> t, w = a.W >> t;
    const int flip = seq_flip(a, im);   // block-uniform
    if (t == 0) {
        const uint8_t* src = a.src + (size_t)(a.gather ? seq_src(a, im) : im) * h * w * 3;
        for (int i = tid; i < h * w; i += kSeqThreads) {
            int sp = i;
            if (flip) {
                const int y = i / w;
                sp = 2 * y * w + w - 1 - i;
            }
            A[3 * i] = src[3 * sp], A[3 * i + 1] = src[3 * sp + 1], A[3 * i + 2] = src[3 * sp + 2];
        }
    } else {
        const int wi = 2 * w, row = w * 3;
        const uint8_t* src = a.src + (size_t)im * (2 * h) * wi * 3;
        const int *bx = a.tabs.bx[t], *kx = a.tabs.kx[t], *by = a.tabs.by[t], *ky = a.tabs.ky[t];
        for (int y0 = 0; y0 < h; y0 += kSeqStripRows) {
            const int y1 = min(y0 + kSeqStripRows, h);
            const int r0 = by[2 * y0], nrows = by[2 * (y1 - 1)] + by[2 * (y1 - 1) + 1] - r0;   // checked on the host
            for (int q = tid; q < nrows * w; q += kSeqThreads) {
                const int ry = q / w, xo = q - ry * w;
                resample_px(src + (size_t)(r0 + ry) * wi * 3, bx[2 * xo], bx[2 * xo + 1], kx + xo * kSeqKsize, Bf + (size_t)q * 3);
            }
            __syncthreads();
            for (int q = tid; q < (y1 - y0) * row; q += kSeqThreads) {
                const int yy = q / row, xb = q - yy * row, yo = y0 + yy;
                const uint8_t v = resample_byte(Bf + (size_t)(by[2 * yo] - r0) * row + xb, row, by[2 * yo + 1], ky + yo * kSeqKsize);
                const int x = xb / 3, c = xb - 3 * x;
                A[((size_t)yo * w + (flip ? w - 1 - x : x)) * 3 + c] = v;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    for (int s = t; s < a.S; ++s) {
        if (s > t) {
            const int hi = h, wi = w;
            h >>= 1, w >>= 1;
            const int row = w * 3;
            const int *bx = a.tabs.bx[s], *kx = a.tabs.kx[s], *by = a.tabs.by[s], *ky = a.tabs.ky[s];
            for (int q = tid; q < hi * w; q += kSeqThreads) {
                const int y = q / w, xo = q - y * w;
                resample_px(A + (size_t)y * wi * 3, bx[2 * xo], bx[2 * xo + 1], kx + xo * kSeqKsize, Bf + (size_t)q * 3);
            }
            __syncthreads();
            for (int q = tid; q < h * row; q += kSeqThreads) {
                const int yo = q / row, xb = q - yo * row;
                const uint8_t v = resample_byte(Bf + (size_t)by[2 * yo] * row + xb, row, by[2 * yo + 1], ky + yo * kSeqKsize);
                const int x = xb / 3, c = xb - 3 * x;
                A[((size_t)yo * w + (flip ? w - 1 - x : x)) * 3 + c] = v;
            }
            __syncthreads();
        }
        const int npix = h * w;
        if (a.steps) {
            // in place, every thread on its own pixels: the steps in front of the contrast, the block's integer luma sum,
            // then the rest -- the same bytes as the whole chain evaluated per pixel (each step ends in 8 bits)
            const JChain ch = jchain_load(a.steps, a.params, seq_jrow(a, im) * a.S + s);
            int mean = 0, first = 0;
            if (ch.c >= 0) {   // block-uniform
                unsigned int acc = 0;
                for (int i = tid; i < npix; i += kSeqThreads) {
                    int r = A[3 * i], g = A[3 * i + 1], b = A[3 * i + 2];
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        if (k < ch.c) jitter_op(r, g, b, ch.op[k], ch.a[k], 0);
                    A[3 * i] = (uint8_t)r, A[3 * i + 1] = (uint8_t)g, A[3 * i + 2] = (uint8_t)b;
                    acc += luma(r, g, b);
                }
                unsigned long long v = acc;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
                if ((tid & 63) == 0) part[tid >> 6] = v;
                __syncthreads();
                unsigned long long sum = 0;
#pragma unroll
                for (int k = 0; k < kSeqThreads / 64; ++k) sum += part[k];
                mean = luma_mean(sum, npix);
                first = ch.c;
                __syncthreads();   // part[] is written again at the next level
            }
            for (int i = tid; i < npix; i += kSeqThreads) {
                int r = A[3 * i], g = A[3 * i + 1], b = A[3 * i + 2];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k >= first) jitter_op(r, g, b, ch.op[k], ch.a[k], mean);
                A[3 * i] = (uint8_t)r, A[3 * i + 1] = (uint8_t)g, A[3 * i + 2] = (uint8_t)b;
            }
        }
        float* o = a.color[s] + (size_t)im * npix * 3;
        float4* pk = (s == 0 && a.packed) ? a.packed + (size_t)im * npix : nullptr;
        for (int i = tid; i < npix; i += kSeqThreads) {   // a thread reads back its own pixels: no barrier needed in front
            const float fr = (float)A[3 * i] / 255.0f, fg = (float)A[3 * i + 1] / 255.0f, fb = (float)A[3 * i + 2] / 255.0f;
            o[i] = fr;
            o[(size_t)npix + i] = fg;
            o[(size_t)2 * npix + i] = fb;
            if (pk) pk[i] = make_float4(fr, fg, fb, 0.f);
        }
        __syncthreads();   // the next level's horizontal pass reads other threads' pixels
    }
}

// LDS bytes of a tail that starts at level t, as (offset of B, total)
static void seq_tail_lds(int H, int W, int S, int t, size_t* b_off, size_t* total) {
    const size_t level = (size_t)(H >> t) * (W >> t) * 3;
    size_t b = t + 1 < S ? level / 2 : 0;                                              // (h_t, w_{t+1}, 3)
    if (t > 0) b = std::max(b, (size_t)kSeqStripSrcRows * (W >> t) * 3);
    *b_off = (level + 15) / 16 * 16;
    *total = *b_off + (b + 15) / 16 * 16;
}

static bool seq_shape_ok(int n, int H, int W, int S) {
    if (n < 1 || n > 20000 || S < 1 || S > DC_MAX_SCALES || H <= 0 || H > 65535 || W <= 0 || W > 65535 || (size_t)H * W > (1u << 28)) return false;
    const int last = 1 << (S - 1);
    return H % last == 0 && W % last == 0;
}

}  // namespace dc

using namespace dc;

extern "C" int dc_data_seq_batch_plan(int items, int n, int H, int W, int S, int jitter, int lds_budget, dc_seq_plan* plan) {
    if (!plan || items < 1 || items > kSeqMaxItems || !seq_shape_ok(n, H, W, S) || lds_budget < 0) return DC_EINVAL;
    if ((long long)items * (jitter ? 3 * n : n + 2) > 65535) return DC_EINVAL;   // one grid row per image
    const size_t budget = lds_budget ? std::min((size_t)lds_budget, (size_t)kSeqLdsCap) : (size_t)kSeqLdsDefault;
    dc_seq_plan p = {};
    p.n_img = items * (jitter ? 3 * n : n + 2);
    p.tail_start = S;
    for (int t = 0; t < S; ++t) {
        size_t b_off, total;
        seq_tail_lds(H, W, S, t, &b_off, &total);
        if (total <= budget) {
            p.tail_start = t;
            p.lds_bytes = (long long)total;
            break;
        }
    }
    for (int s = 1; s < S; ++s) p.table_len += (long long)(2 + kSeqKsize) * ((H >> s) + (W >> s));
    // scratch: [sums | u[0] .. u[tail_start - 1] | horizontal pass | resized level] -- the last two only for tiled levels >= 1
    size_t bytes = (size_t)p.n_img * S * sizeof(unsigned long long);
    for (int s = 0; s < p.tail_start && s + 1 < S; ++s) bytes += ((size_t)p.n_img * (H >> s) * (W >> s) * 3 + 15) / 16 * 16;
    if (p.tail_start > 1)
        bytes += ((size_t)p.n_img * H * (W >> 1) * 3 + 15) / 16 * 16 + ((size_t)p.n_img * (H >> 1) * (W >> 1) * 3 + 15) / 16 * 16;
    p.scratch_bytes = (long long)bytes;
    *plan = p;
    return DC_OK;
}

extern "C" int dc_data_seq_plan(int n, int H, int W, int S, int jitter, int lds_budget, dc_seq_plan* plan) {
    return dc_data_seq_batch_plan(1, n, H, W, S, jitter, lds_budget, plan);
}

extern "C" int dc_data_seq_batch_levels(const uint8_t* frames, int items, int n, int H, int W, int S, const int* flips,
                                        float* const* color, float* packed, const int* steps, const float* params, const int* tab_host,
                                        const int* tab_dev, size_t tab_len, void* scratch, size_t scratch_bytes, int lds_budget,
                                        void* stream) {
    if (!frames || !flips || !color || !packed || ((size_t)packed & 15) || !scratch || ((size_t)scratch & 15)) return DC_EINVAL;
    if ((steps == nullptr) != (params == nullptr)) return DC_EINVAL;   // a step is jittered as a whole or not at all
    dc_seq_plan plan;
    if (dc_data_seq_batch_plan(items, n, H, W, S, steps != nullptr, lds_budget, &plan) != DC_OK) return DC_EINVAL;
    for (int s = 0; s < S; ++s)
        if (!color[s]) return DC_EINVAL;
    if (S > 1 && (!tab_host || !tab_dev)) return DC_EINVAL;
    if ((long long)tab_len != plan.table_len) return DC_EINVAL;
    if (scratch_bytes < (size_t)plan.scratch_bytes) return DC_EWORKSPACE;

    SeqArgs a = {};
    a.n = n, a.S = S, a.H = H, a.W = W, a.items = items;
    for (int i = 0; i < items; ++i)
        if (flips[i]) a.flips[i >> 5] |= 1u << (i & 31);
    a.steps = steps, a.params = params;
    a.packed = (float4*)packed;
    for (int s = 0; s < S; ++s) a.color[s] = color[s];
    // tables of level s: [bounds_x (w, 2) | kk_x (w, 13) | bounds_y (h, 2) | kk_y (h, 13)]; every tap checked on the host copy
    size_t off = 0;
    for (int s = 1; s < S; ++s) {
        const int h = H >> s, w = W >> s;
        a.tabs.bx[s] = tab_dev + off;
        a.tabs.kx[s] = tab_dev + off + 2 * (size_t)w;
        a.tabs.by[s] = tab_dev + off + (size_t)(2 + kSeqKsize) * w;
        a.tabs.ky[s] = a.tabs.by[s] + 2 * (size_t)h;
        const int* bx = tab_host + off;
        const int* by = tab_host + off + (size_t)(2 + kSeqKsize) * w;
        for (int o = 0; o < w; ++o)
            if (bx[2 * o] < 0 || bx[2 * o + 1] < 0 || bx[2 * o + 1] > kSeqKsize || bx[2 * o] + bx[2 * o + 1] > 2 * w) return DC_EINVAL;
        for (int o = 0; o < h; ++o)
            if (by[2 * o] < 0 || by[2 * o + 1] < 0 || by[2 * o + 1] > kSeqKsize || by[2 * o] + by[2 * o + 1] > 2 * h) return DC_EINVAL;
        for (int y0 = 0; y0 < h; y0 += kSeqStripRows) {   // a strip's source rows: a window that starts at its first row and fits B
            const int y1 = std::min(y0 + kSeqStripRows, h), r0 = by[2 * y0];
            for (int o = y0; o < y1; ++o)
                if (by[2 * o] < r0 || by[2 * o] + by[2 * o + 1] - r0 > kSeqStripSrcRows ||
                    by[2 * o] + by[2 * o + 1] > by[2 * (y1 - 1)] + by[2 * (y1 - 1) + 1])
                    return DC_EINVAL;
        }
        off += (size_t)(2 + kSeqKsize) * (h + w);
    }

    // ---- launches ----
    hipStream_t st = (hipStream_t)stream;
    const int N = plan.n_img, t = plan.tail_start;
    uint8_t* base = (uint8_t*)scratch;
    a.sums = (unsigned long long*)base;
    size_t pos = (size_t)N * S * sizeof(unsigned long long);
    if (steps && t > 0 && hipMemsetAsync(a.sums, 0, pos, st) != hipSuccess) return DC_ELAUNCH;
    uint8_t* u[DC_MAX_SCALES] = {};
    for (int s = 0; s < t && s + 1 < S; ++s) {
        u[s] = base + pos;
        pos += ((size_t)N * (H >> s) * (W >> s) * 3 + 15) / 16 * 16;
    }
    uint8_t* mid = base + pos;
    uint8_t* resized = mid + ((size_t)N * H * (W >> 1) * 3 + 15) / 16 * 16;
    for (int s = 0; s < t; ++s) {
        const int h = H >> s, w = W >> s;
        a.level = s;
        a.gather = s == 0;
        a.u8 = u[s];
        if (s == 0) {
            a.src = frames;
        } else {
            int rc = dc_data_resize_axis(u[s - 1], mid, N, 2 * h, 2 * w, w, 1, a.tabs.bx[s], a.tabs.kx[s], kSeqKsize, nullptr, stream);
            if (rc == DC_OK) rc = dc_data_resize_axis(mid, resized, N, 2 * h, w, h, 0, a.tabs.by[s], a.tabs.ky[s], kSeqKsize, nullptr, stream);
            if (rc != DC_OK) return rc;
            a.src = resized;
        }
        const int npix = h * w;
        if (steps) hipLaunchKernelGGL(seq_sum_kernel, dim3(std::min((npix + 255) / 256, 64), N), dim3(256), 0, st, a);
        hipLaunchKernelGGL(seq_finish_kernel, dim3(std::min((npix + 255) / 256, 1024), N), dim3(256), 0, st, a);
    }
    if (t < S) {
        size_t b_off, total;
        seq_tail_lds(H, W, S, t, &b_off, &total);
        static const bool attr = set_max_dynamic_lds(seq_tail_kernel, kSeqLdsCap);
        if (!attr) return DC_ELAUNCH;
        a.level = t;
        a.gather = t == 0;
        a.u8 = nullptr;
        a.src = t == 0 ? frames : u[t - 1];
        a.b_off = (int)b_off;
        hipLaunchKernelGGL(seq_tail_kernel, dim3(N), dim3(kSeqThreads), total, st, a);
    }
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" int dc_data_seq_levels(const uint8_t* frames, int n, int H, int W, int S, int flip, float* const* color, float* packed,
                                  const int* steps, const float* params, const int* tab_host, const int* tab_dev, size_t tab_len,
                                  void* scratch, size_t scratch_bytes, int lds_budget, void* stream) {
    const int flips[1] = {flip};
    return dc_data_seq_batch_levels(frames, 1, n, H, W, S, flips, color, packed, steps, params, tab_host, tab_dev, tab_len, scratch,
                                    scratch_bytes, lds_budget, stream);
}
