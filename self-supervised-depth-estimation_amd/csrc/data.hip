// Per-item data step on the device (reference datasets/mono_dataset.py:92-118 `preprocess`, :139-211
// `__getitem__`): horizontal flip, the Lanczos resize pyramid, ColorJitter and ToTensor for a whole batch of decoded frames
// that already sit in HBM as uint8 HWC.  The arithmetic is Pillow's (libImaging Resample.c / Blend.c / Convert.c) and
// torchvision's functional_pil glue, restated so that every byte equals what the reference's CPU workers produce:
//   * resize: two 8-bit passes (horizontal, then vertical), 22-bit fixed-point coefficients computed on the host in double
//     (dc_resample_table), int32 accumulation with rounding, clip to 8 bits after each pass;
//   * ColorJitter: brightness / contrast / saturation = Image.blend(degenerate, image, factor) in single precision with
//     truncation (interpolation) or clip + truncation (extrapolation); contrast needs the integer mean of the L image
//     (exact 64-bit sum); hue = uint8 shift of H between Pillow's float/double RGB<->HSV conversions;
//   * ToTensor: CHW float32, true division by 255.
// HBM-bound byte work: no LDS staging needed beyond what L2 gives the overlapping filter taps; one thread per output pixel.
// The per-pixel arithmetic (clip, luma, blend, HSV, the jitter step) lives in data_dev.h, shared with seqdata.hip.
#include "data_dev.h"

#include <math.h>

#include <algorithm>

#pragma clang fp contract(off)   // Pillow's C is compiled without fused multiply-adds; every rounding below is load-bearing

namespace dc {

// src (n, H, Wi, 3) -> dst (n, H, Wo, 3); flip[img] != 0 reads the row mirrored (FLIP_LEFT_RIGHT before the resize)
__global__ __launch_bounds__(256) void data_resize_x_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int Wi, int Wo,
                                                           const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                           const uint8_t* __restrict__ flip) {
    const int img = blockIdx.z, y = blockIdx.y, xo = blockIdx.x * 256 + threadIdx.x;
    if (xo >= Wo) return;
    const int x0 = bounds[2 * xo], n = bounds[2 * xo + 1];
    const int* k = kk + (size_t)xo * ksize;
    const uint8_t* row = src + ((size_t)img * H + y) * Wi * 3;
    const bool mirror = flip && flip[img];
    int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < n; ++j) {
        const int sx = mirror ? Wi - 1 - (x0 + j) : x0 + j;
        const uint8_t* p = row + (size_t)sx * 3;
        const int c = k[j];
        a0 += c * p[0];
        a1 += c * p[1];
        a2 += c * p[2];
    }
    uint8_t* o = dst + (((size_t)img * H + y) * Wo + xo) * 3;
    o[0] = clip8(a0);
    o[1] = clip8(a1);
    o[2] = clip8(a2);
}

// src (n, Hi, row) -> dst (n, Ho, row), row = W * 3 bytes; one thread per output byte (coalesced along the row)
__global__ __launch_bounds__(256) void data_resize_y_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int Hi, int Ho, int row,
                                                           const int* __restrict__ bounds, const int* __restrict__ kk, int ksize) {
    const int img = blockIdx.z, yo = blockIdx.y, xb = blockIdx.x * 256 + threadIdx.x;
    if (xb >= row) return;
    const int y0 = bounds[2 * yo], n = bounds[2 * yo + 1];
    const int* k = kk + (size_t)yo * ksize;
    const uint8_t* p = src + ((size_t)img * Hi + y0) * row + xb;
    int a = 1 << (kPrecisionBits - 1);
    for (int j = 0; j < n; ++j) a += k[j] * p[(size_t)j * row];
    dst[((size_t)img * Ho + yo) * row + xb] = clip8(a);
}

// same as above when the horizontal pass is skipped but the image is flipped: plain mirrored copy
__global__ __launch_bounds__(256) void data_flip_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W,
                                                       const uint8_t* __restrict__ flip) {
    const int img = blockIdx.z, y = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const int sx = (flip && flip[img]) ? W - 1 - x : x;
    const uint8_t* p = src + (((size_t)img * H + y) * W + sx) * 3;
    uint8_t* o = dst + (((size_t)img * H + y) * W + x) * 3;
    o[0] = p[0];
    o[1] = p[1];
    o[2] = p[2];
}

// ---- ragged batch: images of DIFFERENT sizes in one packed buffer, one launch per pass -----------------------------------
// A shuffled KITTI batch mixes five native sizes; each image carries its own descriptor (offsets, size, coefficient table)
// and the arithmetic of the two kernels above is repeated per image.  Every descriptor load and every early return is
// block-uniform (blockIdx only).  table < 0: that image already has the target size along the axis -> plain (x: or
// mirrored) copy in the same launch, where Pillow skips the pass.
// width pass: (Hi, Wi) at src_off -> (Hi, Wo) at dst_off; grid (ceil(Wo / 256), max Hi, n)
__global__ __launch_bounds__(256) void data_ragged_x_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                           const dc_ragged_img* __restrict__ desc, int Wo,
                                                           const dc_ragged_table* __restrict__ tab, const int* __restrict__ bounds_all,
                                                           const int* __restrict__ kk_all) {
    const dc_ragged_img d = desc[blockIdx.z];
    const int y = blockIdx.y, xo = blockIdx.x * 256 + threadIdx.x;
    if (y >= d.Hi) return;   // rows above this image's own height
    if (xo >= Wo) return;
    const uint8_t* row = src + (size_t)d.src_off + (size_t)y * d.Wi * 3;
    uint8_t* o = dst + (size_t)d.dst_off + ((size_t)y * Wo + xo) * 3;
    const bool mirror = d.flip != 0;
    if (d.table < 0) {       // Wi == Wo (checked on the host)
        const uint8_t* p = row + (size_t)(mirror ? Wo - 1 - xo : xo) * 3;
        o[0] = p[0];
        o[1] = p[1];
        o[2] = p[2];
        return;
    }
    const dc_ragged_table t = tab[d.table];
    const int* bounds = bounds_all + t.bounds_off;
    const int x0 = bounds[2 * xo], n = bounds[2 * xo + 1];
    const int* k = kk_all + t.kk_off + (size_t)xo * t.ksize;
    int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < n; ++j) {
        const int sx = mirror ? d.Wi - 1 - (x0 + j) : x0 + j;
        const uint8_t* p = row + (size_t)sx * 3;
        const int c = k[j];
        a0 += c * p[0];
        a1 += c * p[1];
        a2 += c * p[2];
    }
    o[0] = clip8(a0);
    o[1] = clip8(a1);
    o[2] = clip8(a2);
}

// height pass: (Hi, Wi) at src_off -> (Ho, Wi) at dst_off, one thread per output byte; grid (ceil(max Wi * 3 / 256), Ho, n)
__global__ __launch_bounds__(256) void data_ragged_y_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                           const dc_ragged_img* __restrict__ desc, int Ho,
                                                           const dc_ragged_table* __restrict__ tab, const int* __restrict__ bounds_all,
                                                           const int* __restrict__ kk_all) {
    const dc_ragged_img d = desc[blockIdx.z];
    const int yo = blockIdx.y, xb = blockIdx.x * 256 + threadIdx.x;
    const int row = d.Wi * 3;
    if (xb >= row) return;
    const uint8_t* base = src + (size_t)d.src_off + xb;
    uint8_t* o = dst + (size_t)d.dst_off + (size_t)yo * row + xb;
    if (d.table < 0) {       // Hi == Ho (checked on the host)
        *o = base[(size_t)yo * row];
        return;
    }
    const dc_ragged_table t = tab[d.table];
    const int* bounds = bounds_all + t.bounds_off;
    const int y0 = bounds[2 * yo], n = bounds[2 * yo + 1];
    const int* k = kk_all + t.kk_off + (size_t)yo * t.ksize;
    const uint8_t* p = base + (size_t)y0 * row;
    int a = 1 << (kPrecisionBits - 1);
    for (int j = 0; j < n; ++j) a += k[j] * p[(size_t)j * row];
    *o = clip8(a);
}


// exact sum of the L image, only for images whose op at this step is CONTRAST
__global__ __launch_bounds__(256) void data_luma_sum_kernel(const uint8_t* __restrict__ img, int npix, const int* __restrict__ steps, int step,
                                                           unsigned long long* __restrict__ sums) {
    const int im = blockIdx.y;
    if (steps[im * 4 + step] != DC_JITTER_CONTRAST) return;
    const uint8_t* p = img + (size_t)im * npix * 3;
    unsigned int acc = 0;   // <= 255 * ceil(npix / threads) per thread: npix < 2^31 / 255 * threads holds for any image here
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) acc += luma(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
    unsigned long long a = acc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(&sums[im], a);
}


__global__ __launch_bounds__(256) void data_jitter_kernel(uint8_t* __restrict__ img, int npix, const int* __restrict__ steps,
                                                         const float* __restrict__ params, int step,
                                                         const unsigned long long* __restrict__ sums) {
    const int im = blockIdx.y;
    const int op = steps[im * 4 + step];
    if (op < 0) return;
    const float a = params[im * 4 + step];
    const int mean = op == DC_JITTER_CONTRAST ? luma_mean(sums[im], npix) : 0;
    uint8_t* base = img + (size_t)im * npix * 3;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
        uint8_t* p = base + (size_t)3 * i;
        int r = p[0], g = p[1], b = p[2];
        jitter_op(r, g, b, op, a, mean);
        p[0] = (uint8_t)r, p[1] = (uint8_t)g, p[2] = (uint8_t)b;
    }
}

// ---- the whole chain of an item in two passes over the uint8 image, nothing written in between ----------------------------
// ColorJitter is four per-pixel operations; only contrast needs something global (the mean of the L image AT THAT POINT of
// the chain).  Pass 1 re-applies the operations in front of the contrast step and sums L (exact integers; skipped for an
// image without a contrast step); pass 2 recomputes the whole chain per pixel and writes BOTH float tensors of ToTensor --
// ("color", s) from the untouched pixel and ("color_aug", s) from the jittered one.  Per scale: 2 launches instead of 14.
__global__ __launch_bounds__(256) void data_chain_sum_kernel(const uint8_t* __restrict__ img, int npix, const int* __restrict__ steps,
                                                            const float* __restrict__ params, unsigned long long* __restrict__ sums) {
    const int im = blockIdx.y;
    const JChain ch = jchain_load(steps, params, im);
    if (ch.c < 0) return;
    const uint8_t* p = img + (size_t)im * npix * 3;
    unsigned int acc = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
        int r = p[3 * i], g = p[3 * i + 1], b = p[3 * i + 2];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < ch.c) jitter_op(r, g, b, ch.op[k], ch.a[k], 0);
        acc += luma(r, g, b);
    }
    unsigned long long a = acc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(&sums[im], a);
}
__global__ __launch_bounds__(256) void data_chain_tensor_kernel(const uint8_t* __restrict__ img, float* __restrict__ color,
                                                               float* __restrict__ color_aug, int npix, const int* __restrict__ steps,
                                                               const float* __restrict__ params, const unsigned long long* __restrict__ sums) {
    const int im = blockIdx.y;
    const JChain ch = jchain_load(steps, params, im);
    const int mean = ch.c >= 0 ? luma_mean(sums[im], npix) : 0;
    const uint8_t* p = img + (size_t)im * npix * 3;
    float* o = color + (size_t)im * npix * 3;
    float* oa = color_aug ? color_aug + (size_t)im * npix * 3 : nullptr;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
        int r = p[3 * i], g = p[3 * i + 1], b = p[3 * i + 2];
        o[i] = (float)r / 255.0f;
        o[(size_t)npix + i] = (float)g / 255.0f;
        o[(size_t)2 * npix + i] = (float)b / 255.0f;
        if (oa) {
#pragma unroll
            for (int k = 0; k < 4; ++k) jitter_op(r, g, b, ch.op[k], ch.a[k], mean);
            oa[i] = (float)r / 255.0f;
            oa[(size_t)npix + i] = (float)g / 255.0f;
            oa[(size_t)2 * npix + i] = (float)b / 255.0f;
        }
    }
}

// (n, H*W, 3) uint8 -> (n, 3, H*W) float32 / 255
__global__ __launch_bounds__(256) void data_to_tensor_kernel(const uint8_t* __restrict__ img, float* __restrict__ out, int npix) {
    const int im = blockIdx.y;
    const uint8_t* p = img + (size_t)im * npix * 3;
    float* o = out + (size_t)im * npix * 3;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
        o[i] = (float)p[3 * i] / 255.0f;
        o[(size_t)npix + i] = (float)p[3 * i + 1] / 255.0f;
        o[(size_t)2 * npix + i] = (float)p[3 * i + 2] / 255.0f;
    }
}

// (n, H*W, 3) uint8 -> (n, H*W, 4) float32 / 255, pixel-interleaved RGBx (x = 0): the layout the photometric kernels gather from
__global__ __launch_bounds__(256) void data_to_rgbx_kernel(const uint8_t* __restrict__ img, float4* __restrict__ out, int npix) {
    const int im = blockIdx.y;
    const uint8_t* p = img + (size_t)im * npix * 3;
    float4* o = out + (size_t)im * npix;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256)
        o[i] = make_float4((float)p[3 * i] / 255.0f, (float)p[3 * i + 1] / 255.0f, (float)p[3 * i + 2] / 255.0f, 0.f);
}
// (n, 3, H*W) float32 -> (n, H*W, 4) float32 RGBx
__global__ __launch_bounds__(256) void pack_rgbx_kernel(const float* __restrict__ x, float4* __restrict__ out, int npix) {
    const int im = blockIdx.y;
    const float* p = x + (size_t)im * npix * 3;
    float4* o = out + (size_t)im * npix;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256)
        o[i] = make_float4(p[i], p[(size_t)npix + i], p[(size_t)2 * npix + i], 0.f);
}

// ---- warm batch: every level of every image gathered from cache slots, two launches --------------------------------------
// A slot holds the UNFLIPPED, already resized pyramid of one frame (level s packed HWC at g.off[s]); an image of the batch is
// (slot, flip).  The Lanczos tables are mirror-symmetric (depthcore/frame_cache.py), so mirroring a cached level on the way
// out equals resizing the mirrored native frame: the row is read in reverse, nothing is pre-flipped.  The arithmetic per
// pixel is that of data_chain_sum_kernel / data_chain_tensor_kernel / data_to_rgbx_kernel; the contrast mean is per image
// AND per level (sums (n_img, num_scales)) and, being an exact integer sum, does not see the mirror.
// grid (blocks of level 0 | level 1 | ..., n_img): the level of a block and every descriptor load are block-uniform.
struct CachedGeom {
    long long off[DC_MAX_SCALES];       // byte offset of level s inside a slot
    float* color[DC_MAX_SCALES];
    float* aug[DC_MAX_SCALES];
    float4* packed;
    int w[DC_MAX_SCALES], npix[DC_MAX_SCALES];
    int blk0[DC_MAX_SCALES + 1];        // first block of level s along grid x
    int num_scales;
};
constexpr int kCachedSumBlocks = 64;
__device__ __forceinline__ int cached_level(const CachedGeom& g, int bx) {
    int s = 0;
#pragma unroll
    for (int t = 1; t < DC_MAX_SCALES; ++t)
        if (t < g.num_scales && bx >= g.blk0[t]) s = t;
    return s;
}
__global__ __launch_bounds__(256) void data_cached_sum_kernel(const uint8_t* __restrict__ arena, const dc_cached_img* __restrict__ desc,
                                                             const CachedGeom g, const int* __restrict__ steps,
                                                             const float* __restrict__ params, unsigned long long* __restrict__ sums) {
    const int im = blockIdx.y;
    const JChain ch = jchain_load(steps, params, im);
    if (ch.c < 0) return;
    const int s = cached_level(g, blockIdx.x);
    const int npix = g.npix[s], stride = (g.blk0[s + 1] - g.blk0[s]) * 256;
    const uint8_t* p = arena + (size_t)desc[im].slot_off + (size_t)g.off[s];
    unsigned int acc = 0;
    for (int i = (blockIdx.x - g.blk0[s]) * 256 + threadIdx.x; i < npix; i += stride) {
        int r = p[3 * i], gg = p[3 * i + 1], b = p[3 * i + 2];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < ch.c) jitter_op(r, gg, b, ch.op[k], ch.a[k], 0);
        acc += luma(r, gg, b);
    }
    unsigned long long a = acc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    // one atomic per block: the adds to one (image, level) word serialise in L2, and with one per wave of a block per 256
    // pixels that chain, not the 3 bytes per pixel, was the whole pass (measured: 198 us for 36 images at 192 x 640)
    __shared__ unsigned long long part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&sums[(size_t)im * g.num_scales + s], part[0] + part[1] + part[2] + part[3]);
}
__global__ __launch_bounds__(256) void data_cached_write_kernel(const uint8_t* __restrict__ arena, const dc_cached_img* __restrict__ desc,
                                                               const CachedGeom g, const int* __restrict__ steps,
                                                               const float* __restrict__ params,
                                                               const unsigned long long* __restrict__ sums) {
    const int im = blockIdx.y;
    const int s = cached_level(g, blockIdx.x);
    const int w = g.w[s], npix = g.npix[s], stride = (g.blk0[s + 1] - g.blk0[s]) * 256;
    const dc_cached_img d = desc[im];
    const bool mirror = d.flip != 0;
    const uint8_t* p = arena + (size_t)d.slot_off + (size_t)g.off[s];
    float* o = g.color[s] + (size_t)im * npix * 3;
    float* oa = g.aug[0] ? g.aug[s] + (size_t)im * npix * 3 : nullptr;
    float4* pk = (s == 0 && g.packed) ? g.packed + (size_t)im * npix : nullptr;
    const JChain ch = jchain_load(oa ? steps : nullptr, params, im);
    const int mean = ch.c >= 0 ? luma_mean(sums[(size_t)im * g.num_scales + s], npix) : 0;
    for (int i = (blockIdx.x - g.blk0[s]) * 256 + threadIdx.x; i < npix; i += stride) {
        int src = i;
        if (mirror) {
            const int y = i / w;
            src = 2 * y * w + w - 1 - i;     // (y, w - 1 - x)
        }
        const uint8_t* q = p + (size_t)3 * src;
        int r = q[0], gg = q[1], b = q[2];
        const float fr = (float)r / 255.0f, fg = (float)gg / 255.0f, fb = (float)b / 255.0f;
        o[i] = fr;
        o[(size_t)npix + i] = fg;
        o[(size_t)2 * npix + i] = fb;
        if (pk) pk[i] = make_float4(fr, fg, fb, 0.f);
        if (oa) {
#pragma unroll
            for (int k = 0; k < 4; ++k) jitter_op(r, gg, b, ch.op[k], ch.a[k], mean);
            oa[i] = (float)r / 255.0f;
            oa[(size_t)npix + i] = (float)gg / 255.0f;
            oa[(size_t)2 * npix + i] = (float)b / 255.0f;
        }
    }
}

// ---- host: Resample.c precompute_coeffs + normalize_coeffs_8bpc, Lanczos (support 3) over the whole axis ----------------
static inline double sinc_filter(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}
static inline double lanczos_filter(double x) { return (-3.0 <= x && x < 3.0) ? sinc_filter(x) * sinc_filter(x / 3) : 0.0; }

}  // namespace dc

using namespace dc;

extern "C" int dc_resample_ksize(int in_size, int out_size) {
    if (in_size <= 0 || out_size <= 0) return 0;
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(3.0 * filterscale) * 2 + 1;
}

extern "C" int dc_resample_table(int in_size, int out_size, int* bounds, int* kk) {
    if (in_size <= 0 || out_size <= 0 || !bounds || !kk) return DC_EINVAL;
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 3.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    const double ss = 1.0 / filterscale;
    double* w = new double[ksize];
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            w[x] = lanczos_filter((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int* k = kk + (size_t)xx * ksize;
        for (int x = 0; x < ksize; ++x) {
            if (x >= xmax) {
                k[x] = 0;
                continue;
            }
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int)(-0.5 + v * (1 << kPrecisionBits)) : (int)(0.5 + v * (1 << kPrecisionBits));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    delete[] w;
    return DC_OK;
}

static bool img_ok(int n, int H, int W) { return n > 0 && n <= 65535 && H > 0 && H <= 65535 && W > 0 && (size_t)n * H * W * 3 < (1ull << 40); }

extern "C" int dc_data_resize_axis(const uint8_t* src, uint8_t* dst, int n_img, int Hi, int Wi, int out_size, int axis, const int* bounds,
                                   const int* kk, int ksize, const uint8_t* flip, void* stream) {
    if (!src || !dst || !bounds || !kk || !img_ok(n_img, Hi, Wi) || out_size <= 0 || out_size > 65535 || (axis != 0 && axis != 1))
        return DC_EINVAL;
    if (ksize != dc_resample_ksize(axis ? Wi : Hi, out_size)) return DC_EINVAL;
    if (axis == 1) {
        hipLaunchKernelGGL(data_resize_x_kernel, dim3((out_size + 255) / 256, Hi, n_img), dim3(256), 0, (hipStream_t)stream, src, dst, Hi, Wi,
                           out_size, bounds, kk, ksize, flip);
    } else {
        if (flip) return DC_EINVAL;   // the mirror belongs to the horizontal pass (or dc_data_flip)
        const int row = Wi * 3;
        hipLaunchKernelGGL(data_resize_y_kernel, dim3((row + 255) / 256, out_size, n_img), dim3(256), 0, (hipStream_t)stream, src, dst, Hi,
                           out_size, row, bounds, kk, ksize);
    }
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" int dc_data_ragged_resize_axis(const uint8_t* src, size_t src_bytes, uint8_t* dst, size_t dst_bytes, const dc_ragged_img* desc_host,
                                          const dc_ragged_img* desc_dev, int n_img, int out_size, int axis, const dc_ragged_table* tab_host,
                                          const dc_ragged_table* tab_dev, int n_tab, const int* bounds_host, const int* bounds_dev,
                                          size_t bounds_len, const int* kk_dev, size_t kk_len, void* stream) {
    if (!src || !dst || src == dst || !desc_host || !desc_dev || n_img <= 0 || n_img > 65535 || out_size <= 0 || out_size > 65535 ||
        (axis != 0 && axis != 1) || n_tab < 0)
        return DC_EINVAL;
    if (n_tab > 0 && (!tab_host || !tab_dev || !bounds_host || !bounds_dev || !kk_dev)) return DC_EINVAL;
    // every table: the size of its axis, and every tap inside [0, in_size) and inside the concatenated arrays
    for (int t = 0; t < n_tab; ++t) {
        const dc_ragged_table& T = tab_host[t];
        if (T.in_size <= 0 || T.in_size > 65535 || T.ksize != dc_resample_ksize(T.in_size, out_size) || T.bounds_off < 0 || T.kk_off < 0 ||
            (size_t)T.bounds_off + 2 * (size_t)out_size > bounds_len || (size_t)T.kk_off + (size_t)out_size * T.ksize > kk_len)
            return DC_EINVAL;
        const int* b = bounds_host + T.bounds_off;
        for (int o = 0; o < out_size; ++o)
            if (b[2 * o] < 0 || b[2 * o + 1] < 0 || b[2 * o + 1] > T.ksize || b[2 * o] + b[2 * o + 1] > T.in_size) return DC_EINVAL;
    }
    // every image: inside both buffers, and its table is the one of its own size
    int max_h = 0, max_w = 0;
    for (int i = 0; i < n_img; ++i) {
        const dc_ragged_img& d = desc_host[i];
        if (d.Hi <= 0 || d.Hi > 65535 || d.Wi <= 0 || d.Wi > 65535 || d.src_off < 0 || d.dst_off < 0) return DC_EINVAL;
        if (axis == 0 && d.flip) return DC_EINVAL;   // the mirror belongs to the width pass
        const size_t in_bytes = (size_t)d.Hi * d.Wi * 3;
        const size_t out_bytes = axis ? (size_t)d.Hi * out_size * 3 : (size_t)out_size * d.Wi * 3;
        if ((size_t)d.src_off > src_bytes || in_bytes > src_bytes - (size_t)d.src_off) return DC_EINVAL;
        if ((size_t)d.dst_off > dst_bytes || out_bytes > dst_bytes - (size_t)d.dst_off) return DC_EINVAL;
        const int in_size = axis ? d.Wi : d.Hi;
        if (d.table < 0 ? in_size != out_size : (d.table >= n_tab || tab_host[d.table].in_size != in_size)) return DC_EINVAL;
        max_h = std::max(max_h, d.Hi);
        max_w = std::max(max_w, d.Wi);
    }
    if (axis == 1)
        hipLaunchKernelGGL(data_ragged_x_kernel, dim3((out_size + 255) / 256, max_h, n_img), dim3(256), 0, (hipStream_t)stream, src, dst,
                           desc_dev, out_size, tab_dev, bounds_dev, kk_dev);
    else
        hipLaunchKernelGGL(data_ragged_y_kernel, dim3((max_w * 3 + 255) / 256, out_size, n_img), dim3(256), 0, (hipStream_t)stream, src, dst,
                           desc_dev, out_size, tab_dev, bounds_dev, kk_dev);
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" int dc_data_flip(const uint8_t* src, uint8_t* dst, int n_img, int H, int W, const uint8_t* flip, void* stream) {
    if (!src || !dst || src == dst || !img_ok(n_img, H, W)) return DC_EINVAL;
    hipLaunchKernelGGL(data_flip_kernel, dim3((W + 255) / 256, H, n_img), dim3(256), 0, (hipStream_t)stream, src, dst, H, W, flip);
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" int dc_data_jitter(uint8_t* img, int n_img, int npix, const int* steps, const float* params, unsigned long long* sums,
                              void* stream) {
    if (!img || !steps || !params || !sums || n_img <= 0 || n_img > 65535 || npix <= 0 || npix > (1 << 28)) return DC_EINVAL;
    const int bx = std::min((npix + 255) / 256, 1024);
    for (int step = 0; step < 4; ++step) {
        if (hipMemsetAsync(sums, 0, sizeof(unsigned long long) * n_img, (hipStream_t)stream) != hipSuccess) return DC_ELAUNCH;
        hipLaunchKernelGGL(data_luma_sum_kernel, dim3(bx, n_img), dim3(256), 0, (hipStream_t)stream, img, npix, steps, step, sums);
        hipLaunchKernelGGL(data_jitter_kernel, dim3(bx, n_img), dim3(256), 0, (hipStream_t)stream, img, npix, steps, params, step, sums);
    }
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" int dc_data_jitter_to_tensor(const uint8_t* img, float* color, float* color_aug, int n_img, int npix, const int* steps,
                                        const float* params, unsigned long long* sums, void* stream) {
    if (!img || !color || n_img <= 0 || n_img > 65535 || npix <= 0 || npix > (1 << 28)) return DC_EINVAL;
    if (color_aug && (!steps || !params || !sums)) return DC_EINVAL;
    const int bx = std::min((npix + 255) / 256, 1024);
    if (color_aug) {
        if (hipMemsetAsync(sums, 0, sizeof(unsigned long long) * n_img, (hipStream_t)stream) != hipSuccess) return DC_ELAUNCH;
        hipLaunchKernelGGL(data_chain_sum_kernel, dim3(bx, n_img), dim3(256), 0, (hipStream_t)stream, img, npix, steps, params, sums);
    }
    hipLaunchKernelGGL(data_chain_tensor_kernel, dim3(bx, n_img), dim3(256), 0, (hipStream_t)stream, img, color, color_aug, npix,
                       color_aug ? steps : (const int*)nullptr, params, (const unsigned long long*)sums);
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" int dc_data_to_tensor(const uint8_t* img, float* out, int n_img, int npix, void* stream) {
    if (!img || !out || n_img <= 0 || n_img > 65535 || npix <= 0 || npix > (1 << 28)) return DC_EINVAL;
    hipLaunchKernelGGL(data_to_tensor_kernel, dim3(std::min((npix + 255) / 256, 1024), n_img), dim3(256), 0, (hipStream_t)stream, img, out,
                       npix);
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" int dc_data_to_rgbx(const uint8_t* img, float* out, int n_img, int npix, void* stream) {
    if (!img || !out || ((size_t)out & 15) || n_img <= 0 || n_img > 65535 || npix <= 0 || npix > (1 << 28)) return DC_EINVAL;
    hipLaunchKernelGGL(data_to_rgbx_kernel, dim3(std::min((npix + 255) / 256, 1024), n_img), dim3(256), 0, (hipStream_t)stream, img,
                       (float4*)out, npix);
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" int dc_pack_rgbx(const float* x, float* out, int n_img, int npix, void* stream) {
    if (!x || !out || ((size_t)out & 15) || n_img <= 0 || n_img > 65535 || npix <= 0 || npix > (1 << 28)) return DC_EINVAL;
    hipLaunchKernelGGL(pack_rgbx_kernel, dim3(std::min((npix + 255) / 256, 1024), n_img), dim3(256), 0, (hipStream_t)stream, x,
                       (float4*)out, npix);
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" int dc_data_cached_levels(const uint8_t* arena, size_t arena_bytes, const dc_cached_img* desc_host, const dc_cached_img* desc_dev,
                                     int n_img, int height, int width, int num_scales, float* const* color, float* const* color_aug,
                                     float* packed, const int* steps, const float* params, unsigned long long* sums, void* stream) {
    if (!arena || !desc_host || !desc_dev || !color || n_img <= 0 || n_img > 65535 || num_scales < 1 || num_scales > DC_MAX_SCALES ||
        height <= 0 || height > 65535 || width <= 0 || width > 65535 || (size_t)height * width > (1u << 28))
        return DC_EINVAL;
    const int last = 1 << (num_scales - 1);
    if (height % last || width % last || ((size_t)packed & 15)) return DC_EINVAL;
    if (color_aug && (!steps || !params || !sums)) return DC_EINVAL;
    CachedGeom g = {};
    g.num_scales = num_scales;
    g.packed = (float4*)packed;
    size_t slot_bytes = 0;
    for (int s = 0; s < num_scales; ++s) {
        if (!color[s] || (color_aug && !color_aug[s])) return DC_EINVAL;
        g.color[s] = color[s];
        g.aug[s] = color_aug ? color_aug[s] : nullptr;
        g.w[s] = width >> s;
        g.npix[s] = (height >> s) * (width >> s);
        g.off[s] = (long long)slot_bytes;
        g.blk0[s + 1] = g.blk0[s] + std::min((g.npix[s] + 255) / 256, 1024);
        slot_bytes += (size_t)g.npix[s] * 3;
    }
    // every image: its whole slot inside the arena
    for (int i = 0; i < n_img; ++i) {
        const dc_cached_img& d = desc_host[i];
        if (d.slot_off < 0 || (size_t)d.slot_off > arena_bytes || slot_bytes > arena_bytes - (size_t)d.slot_off) return DC_EINVAL;
    }
    const dim3 grid(g.blk0[num_scales], n_img);
    if (color_aug) {
        if (hipMemsetAsync(sums, 0, sizeof(unsigned long long) * n_img * num_scales, (hipStream_t)stream) != hipSuccess) return DC_ELAUNCH;
        // the sum pass walks each level with at most kCachedSumBlocks blocks per image (grid-stride): few atomics per word
        CachedGeom gs = g;
        for (int s = 0; s < num_scales; ++s) gs.blk0[s + 1] = gs.blk0[s] + std::min((g.npix[s] + 255) / 256, kCachedSumBlocks);
        hipLaunchKernelGGL(data_cached_sum_kernel, dim3(gs.blk0[num_scales], n_img), dim3(256), 0, (hipStream_t)stream, arena, desc_dev, gs,
                           steps, params, sums);
    }
    hipLaunchKernelGGL(data_cached_write_kernel, grid, dim3(256), 0, (hipStream_t)stream, arena, desc_dev, g,
                       color_aug ? steps : (const int*)nullptr, params, (const unsigned long long*)sums);
    DC_CHECK_LAUNCH();
    return DC_OK;
}
