// Device arithmetic of the data step, shared by data.hip (per-item batches) and seqdata.hip (sequences): Pillow's 8-bit
// resampling clip, Convert.c's luma and RGB<->HSV, Blend.c's blend, and torchvision's ColorJitter step built from them.
// One definition, so that both translation units produce the same bytes.
#pragma once
#include "dc_common.h"

#include <math.h>

#pragma clang fp contract(off)   // Pillow's C is compiled without fused multiply-adds; every rounding below is load-bearing

namespace dc {

constexpr int kPrecisionBits = 32 - 8 - 2;   // Resample.c PRECISION_BITS

__device__ __forceinline__ uint8_t clip8(int acc) {
    const int v = acc >> kPrecisionBits;
    return (uint8_t)min(max(v, 0), 255);
}

__device__ __forceinline__ int luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }   // Convert.c L24

// Blend.c: (UINT8)(in1 + alpha * (in2 - in1)), in1 = degenerate; outside [0, 1]: clip, then truncate
__device__ __forceinline__ uint8_t blend(int d, int x, float a, bool interp) {
    float m = a * (float)(x - d);
    asm volatile("" : "+v"(m));   // the product is rounded before the add: HIP's __fmul_rn / __fadd_rn are plain operators that
    const float t = (float)d + m;  // the compiler fuses, and a fused multiply-add differs whenever a * (x - d) is near an integer
    if (interp) return (uint8_t)(int)t;
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (uint8_t)(int)t);
}

// Convert.c rgb2hsv_row: float variables, double literals (see oracle/data_ref.py)
__device__ __forceinline__ void rgb2hsv(int r, int g, int b, int& uh, int& us, int& uv) {
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    uv = maxc;
    if (minc == maxc) {
        uh = 0;
        us = 0;
        return;
    }
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc)
        h = bc - gc;
    else if (g == maxc)
        h = (float)(2.0 + (double)rc - (double)bc);
    else
        h = (float)(4.0 + (double)gc - (double)rc);
    double hd = (double)h / 6.0 + 1.0;          // in [5/6, 11/6]
    hd = hd >= 1.0 ? hd - 1.0 : hd;             // fmod(., 1.0), exact
    h = (float)hd;
    uh = min(max((int)((double)h * 255.0), 0), 255);
    us = min(max((int)((double)s * 255.0), 0), 255);
}

// Convert.c hsv2rgb
__device__ __forceinline__ void hsv2rgb(int h, int s, int v, int& r, int& g, int& b) {
    if (s == 0) {
        r = g = b = v;
        return;
    }
    const double fh = (double)(float)h * 6.0 / 255.0;
    const int i = (int)floor(fh);
    const double f = (double)(float)(fh - (double)(float)i);
    const double fs = (double)(float)((double)(float)s / 255.0);
    const double vf = (double)(float)v;
    const int p = min(max((int)round(vf * (1.0 - fs)), 0), 255);
    const int q = min(max((int)round(vf * (1.0 - fs * f)), 0), 255);
    const int t = min(max((int)round(vf * (1.0 - fs * (1.0 - f))), 0), 255);
    switch (i % 6) {
        case 0: r = v, g = t, b = p; break;
        case 1: r = q, g = v, b = p; break;
        case 2: r = p, g = v, b = t; break;
        case 3: r = p, g = q, b = v; break;
        case 4: r = t, g = p, b = v; break;
        default: r = v, g = p, b = q; break;
    }
}

// one ColorJitter operation on one pixel (the arithmetic of dc_data_jitter and of every fused chain kernel)
__device__ __forceinline__ void jitter_op(int& r, int& g, int& b, int op, float a, int mean) {
    if (op == DC_JITTER_HUE) {
        int h, s, v;
        rgb2hsv(r, g, b, h, s, v);
        h = (h + (int)a) & 0xFF;
        hsv2rgb(h, s, v, r, g, b);
    } else if (op >= 0) {
        const bool interp = a >= 0.f && a <= 1.f;
        int d0 = 0;
        if (op == DC_JITTER_CONTRAST) d0 = mean;
        else if (op == DC_JITTER_SATURATION) d0 = luma(r, g, b);
        r = blend(d0, r, a, interp);
        g = blend(d0, g, a, interp);
        b = blend(d0, b, a, interp);
    }
}
__device__ __forceinline__ int luma_mean(unsigned long long sum, int npix) { return (int)((double)sum / (double)npix + 0.5); }   // int(ImageStat mean + 0.5)

// the four steps of one image's ColorJitter; c = the position of the contrast step (the only one that needs a global value)
struct JChain { int op[4]; float a[4]; int c; };
__device__ __forceinline__ JChain jchain_load(const int* steps, const float* params, int im) {
    JChain ch;
    ch.c = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ch.op[k] = steps ? steps[im * 4 + k] : DC_JITTER_NONE;
        ch.a[k] = steps ? params[im * 4 + k] : 0.f;
        if (ch.op[k] == DC_JITTER_CONTRAST && ch.c < 0) ch.c = k;
    }
    return ch;
}

// one output pixel of the horizontal 8-bit pass: `n` taps from source pixel x0 of an HWC row (Resample.c ImagingResampleHorizontal_8bpc)
__device__ __forceinline__ void resample_px(const uint8_t* row, int x0, int n, const int* k, uint8_t* o) {
    int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < n; ++j) {
        const uint8_t* p = row + (size_t)(x0 + j) * 3;
        const int c = k[j];
        a0 += c * p[0];
        a1 += c * p[1];
        a2 += c * p[2];
    }
    o[0] = clip8(a0);
    o[1] = clip8(a1);
    o[2] = clip8(a2);
}
// one output byte of the vertical pass: `n` taps `row` bytes apart
__device__ __forceinline__ uint8_t resample_byte(const uint8_t* p, int row, int n, const int* k) {
    int a = 1 << (kPrecisionBits - 1);
    for (int j = 0; j < n; ++j) a += k[j] * p[(size_t)j * row];
    return clip8(a);
}

}  // namespace dc
