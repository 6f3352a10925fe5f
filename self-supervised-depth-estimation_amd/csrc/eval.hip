// Depth evaluation of a trained model, the prediction side of evaluate_depth.py (include/depthcore.h: dc_flip_concat,
// dc_disp_post_process, dc_depth_png16).  The scoring is dc_depth_errors (metrics.hip).  All three are streaming kernels,
// one output element per thread and grid-stride, coalesced along W on the writes.
#include "dc_common.h"

namespace dc {

constexpr int EV_THREADS = 256;
constexpr int EV_MAX_BLOCKS = 8192;

static inline int ev_blocks(size_t n) { return (int)std::min<size_t>((n + EV_THREADS - 1) / EV_THREADS, EV_MAX_BLOCKS); }

// evaluate_depth.py:123 torch.cat((x, torch.flip(x, [3])), 0): element i of x goes to out[i] and, mirrored, to out[n + i']
__global__ __launch_bounds__(EV_THREADS) void flip_concat_kernel(const float* __restrict__ x, float* __restrict__ out, size_t n, int W) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const size_t row = i / (size_t)W;
        const int col = (int)(i - row * (size_t)W);
        out[i] = x[i];
        out[n + i] = x[row * (size_t)W + (size_t)(W - 1 - col)];
    }
}

// np.linspace(0, 1, w)[j]: j * (1.0 / (w - 1)) + 0.0, the last element exactly 1.0, [0.0] for w == 1
__device__ __forceinline__ double ev_linspace(int j, int w) {
    if (w == 1) return 0.0;
    if (j == w - 1) return 1.0;
    return (double)j * (1.0 / (double)(w - 1));
}

// (1.0 - np.clip(20 * (l - 0.05), 0, 1)) of evaluate_depth.py:54, fp64
__device__ __forceinline__ double ev_lmask(int j, int w) {
#pragma clang fp contract(off)
    const double t = 20.0 * (ev_linspace(j, w) - 0.05);
    return 1.0 - fmin(fmax(t, 0.0), 1.0);
}

// out (B,1,h,w) from disp (2B,1,h,w): scaled disparity of both halves (the second mirrored back, as pred_disp[N:, :, ::-1]),
// then batch_post_process_disparity (evaluate_depth.py:48-56) in numpy's types and order
__global__ __launch_bounds__(EV_THREADS) void disp_post_process_kernel(const float* __restrict__ disp, float* __restrict__ out, size_t n,
                                                                       int w, float lo, float rng) {
#pragma clang fp contract(off)
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const size_t row = i / (size_t)w;
        const int j = (int)(i - row * (size_t)w);
        const float l = disp_scaled(disp[i], lo, rng);
        const float r = disp_scaled(disp[n + row * (size_t)w + (size_t)(w - 1 - j)], lo, rng);
        const float m = 0.5f * (l + r);                                   // fp32: numpy 0.5 * (l_disp + r_disp)
        const double lm = ev_lmask(j, w), rm = ev_lmask(w - 1 - j, w);    // r_mask = l_mask[:, :, ::-1]
        const double v = rm * (double)l + lm * (double)r + (1.0 - lm - rm) * (double)m;
        out[i] = (float)v;
    }
}

// evaluate_depth.py:166-169: uint16(clip(scale / resize(disp), 0, 80) * 256)
__global__ __launch_bounds__(EV_THREADS) void depth_png16_kernel(const float* __restrict__ disp, uint16_t* __restrict__ out, size_t n,
                                                                 int h, int w, int Ho, int Wo, float ry, float rx, float scale) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t plane = (size_t)Ho * Wo;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const size_t img = i / plane;
        const int p = (int)(i - img * plane);
        const int oy = p / Wo, ox = p - oy * Wo;
        const float v = bilinear_at(disp + img * (size_t)h * w, h, w, Ho, Wo, oy, ox, ry, rx);
        const float depth = fminf(fmaxf(scale / v, 0.f), 80.f);            // np.clip; NaN -> 0
        out[i] = (uint16_t)(unsigned)(depth * 256.f);                       // in [0, 20480]: truncation, as np.uint16
    }
}

}  // namespace dc

using namespace dc;

extern "C" int dc_flip_concat(const float* x, float* out, int B, int C, int H, int W, void* stream) {
    if (!x || !out || B <= 0 || C <= 0 || H <= 0 || W <= 0) return DC_EINVAL;
    const size_t n = (size_t)B * C * H * W;
    hipLaunchKernelGGL(flip_concat_kernel, dim3(ev_blocks(n)), dim3(EV_THREADS), 0, (hipStream_t)stream, x, out, n, W);
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" int dc_disp_post_process(const float* disp, float* out, int B, int h, int w, float min_depth, float max_depth, void* stream) {
    if (!disp || !out || B <= 0 || h <= 0 || w <= 0 || !(min_depth > 0.f) || !(max_depth > min_depth)) return DC_EINVAL;
    const float lo = 1.f / max_depth, rng = 1.f / min_depth - 1.f / max_depth;     // as dc_disp_to_depth_fwd
    const size_t n = (size_t)B * h * w;
    hipLaunchKernelGGL(disp_post_process_kernel, dim3(ev_blocks(n)), dim3(EV_THREADS), 0, (hipStream_t)stream, disp, out, n, w, lo, rng);
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" int dc_depth_png16(const float* disp, uint16_t* out, int N, int h, int w, int Ho, int Wo, float scale, void* stream) {
    if (!disp || !out || N <= 0 || h <= 0 || w <= 0 || Ho <= 0 || Wo <= 0 || (long long)Ho * Wo >= 0x7fffffffLL) return DC_EINVAL;
    const size_t n = (size_t)N * Ho * Wo;
    const float ry = (float)h / (float)Ho, rx = (float)w / (float)Wo;              // as dc_upsample_bilinear_fwd
    hipLaunchKernelGGL(depth_png16_kernel, dim3(ev_blocks(n)), dim3(EV_THREADS), 0, (hipStream_t)stream, disp, out, n, h, w, Ho, Wo, ry,
                       rx, scale);
    DC_CHECK_LAUNCH();
    return DC_OK;
}
