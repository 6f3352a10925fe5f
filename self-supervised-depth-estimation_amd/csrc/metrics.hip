// Depth metrics of validation: Trainer.compute_depth_losses (reference trainer.py:624-652) and the two masks of evaluate_depth.py:
// 190-235 (the Eigen crop; gt > 0 on the whole frame), scored as layers.compute_depth_errors (layers.py:251-269).
// include/depthcore.h: dc_depth_errors.
//
// Every pass walks the crop rectangle of every image (grid (blocks per image, B)) and re-derives, per pixel, the mask from gt
// and -- where it passes -- the prediction: the bilinear upsample of dc_upsample_bilinear_fwd (bilinear_at), the protocol's
// depth transform and clamp.  Nothing is compacted.
//   zero                          histograms, selection state
//   hist(0) select(0)             12-bit digit (key bits 31..20) of every group's gt and pred keys -> n, the digit holding
//   hist(1) select(1)             rank (n-1)/2, the next 12 bits (19..8) among the keys with that prefix, the last 8 (7..0):
//   hist(2) select(2)             the exact key of the lower middle, and how many keys are below / equal to it
//   upper (eigen)                 numpy's upper middle when n is even and it is not a tie: min key above the lower middle
//   metrics                       ratio of medians, scale, clamp, fp64 per-block partials of the seven sums
//   finalize                      one block per group: partials in a fixed order -> out, ratios, status
// Histograms and the min are integer atomics (order-independent); float sums never use atomics: reproducible bit for bit.
#include "dc_common.h"

namespace dc {

constexpr int MT_THREADS = 256;
constexpr int MT_PPT = 8;                              // crop pixels per thread per block
constexpr int MT_TILE = MT_THREADS * MT_PPT;
constexpr int MT_BINS = 4096;
constexpr int MT_NSUM = 8;                             // abs_rel, sq_rel, sq, sq_log, a1, a2, a3 counts, n

struct MtState {                                       // one per (group, gt | pred) selection stream
    unsigned n, rank, prefix, less, key_lo, need_hi, min_above, pad;
};

struct MtArgs {
    const float* pred;
    const float* gt;
    int B, h, w, Hg, Wg, eigen, gtpos, y0, y1, x0, x1, nbx, scaling;   // eigen: evaluate_depth.py's per-image protocol (either mask)
    float ry, rx, scale_factor;
};

// order-preserving map of fp32 onto uint32 (positive floats keep their bit pattern's order; negatives are reversed below them)
__device__ __forceinline__ unsigned mt_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float mt_val(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// crop pixel j of image b: the mask, and (where it passes) gt and the prediction before median scaling
__device__ __forceinline__ bool mt_pixel(const MtArgs& a, int b, int j, float& g, float& p) {
    const int cw = a.x1 - a.x0;
    const int oy = a.y0 + j / cw, ox = a.x0 + j % cw;
    g = a.gt[((size_t)b * a.Hg + oy) * a.Wg + ox];
    const bool ok = (a.eigen && !a.gtpos) ? (g > 1e-3f && g < 80.f) : (g > 0.f);
    if (!ok) return false;
    const float v = bilinear_at(a.pred + (size_t)b * a.h * a.w, a.h, a.w, a.Hg, a.Wg, oy, ox, a.ry, a.rx);
    if (a.eigen) p = (1.0f / v) * a.scale_factor;              // evaluate_depth.py:203, 219
    else p = fminf(fmaxf(v, 1e-3f), 80.f);                     // trainer.py:630-631
    return true;
}

__global__ __launch_bounds__(256) void mt_zero_kernel(unsigned* p, size_t n, MtState* st, int S) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = 0u;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < S; s += (int)stride) {
        MtState z = {};
        z.min_above = 0xffffffffu;
        st[s] = z;
    }
}

// pass 0: bin = key >> 20 of every masked key;  pass 1: (key >> 8) & 0xfff of keys whose top 12 bits are the selected prefix;
// pass 2: key & 0xff of keys whose top 24 bits are.  LDS histograms of the block's two streams, flushed with integer atomics.
template <int PASS>
__global__ __launch_bounds__(MT_THREADS) void mt_hist_kernel(MtArgs a, unsigned* __restrict__ hist, const MtState* __restrict__ st) {
    __shared__ unsigned sh[2 * MT_BINS];
    constexpr int NB = PASS == 2 ? 256 : MT_BINS;
    const int b = blockIdx.y, grp = a.eigen ? b : 0;
    for (int i = threadIdx.x; i < 2 * NB; i += MT_THREADS) sh[i] = 0u;
    unsigned pre[2] = {0u, 0u};
    if (PASS > 0) { pre[0] = st[2 * grp].prefix; pre[1] = st[2 * grp + 1].prefix; }
    __syncthreads();
    const int npix = (a.y1 - a.y0) * (a.x1 - a.x0);
    const int j0 = blockIdx.x * MT_TILE;
    for (int k = 0; k < MT_PPT; ++k) {
        const int j = j0 + k * MT_THREADS + threadIdx.x;
        float g, p;
        if (j >= npix || !mt_pixel(a, b, j, g, p)) continue;
        const unsigned key[2] = {mt_key(g), mt_key(p)};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (PASS == 0) atomicAdd(&sh[s * NB + (key[s] >> 20)], 1u);
            else if (PASS == 1) { if ((key[s] >> 20) == pre[s]) atomicAdd(&sh[s * NB + ((key[s] >> 8) & 0xfffu)], 1u); }
            else { if ((key[s] >> 8) == pre[s]) atomicAdd(&sh[s * NB + (key[s] & 0xffu)], 1u); }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * NB; i += MT_THREADS) {
        const unsigned c = sh[i];
        if (c) atomicAdd(&hist[(size_t)(2 * grp + i / NB) * MT_BINS + (i % NB)], c);
    }
}

// one block per stream: the bin holding the stream's rank.  Integer arithmetic throughout.
template <int PASS>
__global__ __launch_bounds__(MT_THREADS) void mt_select_kernel(const unsigned* __restrict__ hist, MtState* __restrict__ st, int eigen) {
    __shared__ unsigned wsum[MT_THREADS / 64];
    constexpr int NB = PASS == 2 ? 256 : MT_BINS, PER = NB / MT_THREADS;
    const int s = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const unsigned* h = hist + (size_t)s * MT_BINS;
    MtState m = st[s];
    if (PASS > 0 && m.n == 0u) return;                           // empty group: nothing to select (status from finalize)
    unsigned c[PER], tot = 0u;
#pragma unroll
    for (int i = 0; i < PER; ++i) { c[i] = h[t * PER + i]; tot += c[i]; }
    // inclusive scan of the per-thread totals: wave scan, then the wave totals
    unsigned inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    unsigned before = inc - tot, all = 0u;
    for (int i = 0; i < MT_THREADS / 64; ++i) {
        if (i < wv) before += wsum[i];
        all += wsum[i];
    }
    if (PASS == 0) {
        m.n = all;
        m.rank = all ? (all - 1u) / 2u : 0u;                      // lower middle: torch.median, and numpy's first of two
        if (all == 0u) {
            if (t == 0) st[s] = m;
            return;
        }
    }
    const unsigned r = m.rank;
    if (r < before || r >= before + tot) return;
    unsigned cum = before;
    int bin = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        if (r < cum + c[i]) { bin = t * PER + i; break; }
        cum += c[i];
    }
    const unsigned eq = h[bin];
    m.rank = r - cum;
    m.less += cum;
    if (PASS == 0) m.prefix = (unsigned)bin;
    else if (PASS == 1) m.prefix = (m.prefix << 12) | (unsigned)bin;
    else {
        m.key_lo = (m.prefix << 8) | (unsigned)bin;
        // numpy, n even: the upper middle (index n/2) ties with the lower one iff more than n/2 keys are <= it
        m.need_hi = (eigen && (m.n & 1u) == 0u && m.less + eq <= m.n / 2u) ? 1u : 0u;
    }
    st[s] = m;
}

// numpy's upper middle where it is not a tie: the smallest key above the lower middle (integer atomicMin)
__global__ __launch_bounds__(MT_THREADS) void mt_upper_kernel(MtArgs a, MtState* __restrict__ st) {
    const int b = blockIdx.y, grp = a.eigen ? b : 0;
    const unsigned need0 = st[2 * grp].need_hi, need1 = st[2 * grp + 1].need_hi;
    if (!need0 && !need1) return;
    const unsigned lo0 = st[2 * grp].key_lo, lo1 = st[2 * grp + 1].key_lo;
    unsigned m0 = 0xffffffffu, m1 = 0xffffffffu;
    const int npix = (a.y1 - a.y0) * (a.x1 - a.x0);
    const int j0 = blockIdx.x * MT_TILE;
    for (int k = 0; k < MT_PPT; ++k) {
        const int j = j0 + k * MT_THREADS + threadIdx.x;
        float g, p;
        if (j >= npix || !mt_pixel(a, b, j, g, p)) continue;
        const unsigned kg = mt_key(g), kp = mt_key(p);
        if (kg > lo0) m0 = min(m0, kg);
        if (kp > lo1) m1 = min(m1, kp);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m0 = min(m0, (unsigned)__shfl_xor((int)m0, o));
        m1 = min(m1, (unsigned)__shfl_xor((int)m1, o));
    }
    if ((threadIdx.x & 63) == 0) {
        if (need0 && m0 != 0xffffffffu) atomicMin(&st[2 * grp].min_above, m0);
        if (need1 && m1 != 0xffffffffu) atomicMin(&st[2 * grp + 1].min_above, m1);
    }
}

__device__ __forceinline__ float mt_median(const MtState& m, int eigen) {
    const float lo = mt_val(m.key_lo);
    if (!eigen || (m.n & 1u)) return lo;
    const float hi = m.need_hi ? mt_val(m.min_above) : lo;
    return (lo + hi) / 2.f;                                     // np.mean of the two middles, in fp32
}

__device__ __forceinline__ float mt_ratio(const MtState* st, int grp, int eigen, int scaling) {
    if (!scaling) return 1.f;
    const MtState g = st[2 * grp], p = st[2 * grp + 1];
    return mt_median(g, eigen) / mt_median(p, eigen);
}

__device__ __forceinline__ double mt_block_sum(double v, double* sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// partial[(b * nbx + bx) * 8 + k]
__global__ __launch_bounds__(MT_THREADS) void mt_metrics_kernel(MtArgs a, const MtState* __restrict__ st, double* __restrict__ part) {
    __shared__ double sm[MT_THREADS / 64];
    const int b = blockIdx.y, grp = a.eigen ? b : 0;
    const float ratio = mt_ratio(st, grp, a.eigen, a.scaling);
    double acc[MT_NSUM] = {0., 0., 0., 0., 0., 0., 0., 0.};
    const int npix = (a.y1 - a.y0) * (a.x1 - a.x0);
    const int j0 = blockIdx.x * MT_TILE;
    for (int k = 0; k < MT_PPT; ++k) {
        const int j = j0 + k * MT_THREADS + threadIdx.x;
        float g, p;
        if (j >= npix || !mt_pixel(a, b, j, g, p)) continue;
        if (a.scaling) p *= ratio;                               // trainer.py:644 / evaluate_depth.py:223
        p = fminf(fmaxf(p, 1e-3f), 80.f);                        // trainer.py:646 / evaluate_depth.py:225-226
        const float th = fmaxf(g / p, p / g);                    // fp32, as the reference
        const double gd = g, pd = p, d = gd - pd, lg = log(gd) - log(pd);
        acc[0] += fabs(d) / gd;
        acc[1] += d * d / gd;
        acc[2] += d * d;
        acc[3] += lg * lg;
        acc[4] += th < 1.25f ? 1. : 0.;
        acc[5] += th < 1.5625f ? 1. : 0.;
        acc[6] += th < 1.953125f ? 1. : 0.;
        acc[7] += 1.;
    }
    double* o = part + ((size_t)b * a.nbx + blockIdx.x) * MT_NSUM;
#pragma unroll
    for (int i = 0; i < MT_NSUM; ++i) {
        const double v = mt_block_sum(acc[i], sm);
        if (threadIdx.x == 0) o[i] = v;
    }
}

// one block per group: its images' partials, thread t summing entries t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(MT_THREADS) void mt_finalize_kernel(MtArgs a, const MtState* __restrict__ st, const double* __restrict__ part,
                                                                 float* __restrict__ out, float* __restrict__ ratios, int* __restrict__ status) {
    __shared__ double sm[MT_THREADS / 64];
    const int grp = blockIdx.x;
    const int first = a.eigen ? grp * a.nbx : 0, count = a.eigen ? a.nbx : a.B * a.nbx;
    double acc[MT_NSUM] = {0., 0., 0., 0., 0., 0., 0., 0.};
    for (int i = threadIdx.x; i < count; i += MT_THREADS) {
        const double* p = part + (size_t)(first + i) * MT_NSUM;
#pragma unroll
        for (int k = 0; k < MT_NSUM; ++k) acc[k] += p[k];
    }
    double tot[MT_NSUM];
#pragma unroll
    for (int k = 0; k < MT_NSUM; ++k) tot[k] = mt_block_sum(acc[k], sm);
    if (threadIdx.x != 0) return;
    const double n = tot[7];
    float* row = out + (size_t)grp * 7;
    if (n == 0.) {
        for (int k = 0; k < 7; ++k) row[k] = __int_as_float(0x7fc00000);
        if (ratios) ratios[grp] = __int_as_float(0x7fc00000);
        status[grp] = DC_EEMPTY;
        return;
    }
    row[0] = (float)(tot[0] / n);
    row[1] = (float)(tot[1] / n);
    row[2] = (float)sqrt(tot[2] / n);
    row[3] = (float)sqrt(tot[3] / n);
    row[4] = (float)(tot[4] / n);
    row[5] = (float)(tot[5] / n);
    row[6] = (float)(tot[6] / n);
    if (ratios) ratios[grp] = mt_ratio(st, grp, a.eigen, a.scaling);
    status[grp] = DC_OK;
}

struct MtLayout {
    int G, S, nbx;
    size_t hist_words, state_off, part_off, bytes;
};

static bool mt_layout(const dc_depth_eval_desc* d, MtArgs& a, MtLayout& L) {
    if (!d || d->B <= 0 || d->h <= 0 || d->w <= 0 || d->Hg <= 0 || d->Wg <= 0 ||
        (d->protocol != DC_EVAL_TRAINER && d->protocol != DC_EVAL_EIGEN && d->protocol != DC_EVAL_GT_POSITIVE))
        return false;
    a.B = d->B; a.h = d->h; a.w = d->w; a.Hg = d->Hg; a.Wg = d->Wg;
    a.eigen = d->protocol != DC_EVAL_TRAINER;
    a.gtpos = d->protocol == DC_EVAL_GT_POSITIVE;
    if (a.gtpos) {                                             // evaluate_depth.py:210-211: the whole frame
        a.y0 = 0; a.y1 = d->Hg; a.x0 = 0; a.x1 = d->Wg;
    } else {
        a.y0 = max(d->crop[0], 0); a.y1 = min(d->crop[1], d->Hg);
        a.x0 = max(d->crop[2], 0); a.x1 = min(d->crop[3], d->Wg);
    }
    if (a.y1 < a.y0) a.y1 = a.y0;
    if (a.x1 < a.x0) a.x1 = a.x0;
    const long long npix = (long long)(a.y1 - a.y0) * (a.x1 - a.x0);
    if (npix >= 0x7fffffffLL - MT_TILE) return false;
    a.nbx = npix ? (int)((npix + MT_TILE - 1) / MT_TILE) : 1;
    a.scaling = d->median_scaling != 0;
    a.scale_factor = d->scale_factor;
    a.ry = (float)d->h / (float)d->Hg;                         // as dc_upsample_bilinear_fwd
    a.rx = (float)d->w / (float)d->Wg;
    L.G = a.eigen ? d->B : 1;
    L.S = 2 * L.G;
    L.nbx = a.nbx;
    L.hist_words = (size_t)3 * L.S * MT_BINS;
    L.state_off = L.hist_words * sizeof(unsigned);
    L.part_off = (L.state_off + (size_t)L.S * sizeof(MtState) + 255) & ~(size_t)255;
    L.bytes = L.part_off + (size_t)d->B * a.nbx * MT_NSUM * sizeof(double);
    return true;
}

}  // namespace dc

using namespace dc;

extern "C" size_t dc_depth_errors_workspace(const dc_depth_eval_desc* d) {
    MtArgs a;
    MtLayout L;
    return mt_layout(d, a, L) ? L.bytes : 0;
}

extern "C" int dc_depth_errors(const dc_depth_eval_desc* d, const float* pred, const float* gt, float* out, void* ws, void* stream) {
    MtArgs a;
    MtLayout L;
    if (!mt_layout(d, a, L) || !pred || !gt || !out || !ws || !d->status) return DC_EINVAL;
    a.pred = pred;
    a.gt = gt;
    hipStream_t st = (hipStream_t)stream;
    unsigned* hist = (unsigned*)ws;
    MtState* state = (MtState*)((char*)ws + L.state_off);
    double* part = (double*)((char*)ws + L.part_off);
    const dim3 grid(L.nbx, a.B);
    if (a.scaling) {
        hipLaunchKernelGGL(mt_zero_kernel, dim3(min((int)((L.hist_words + 255) / 256), 1024)), dim3(256), 0, st, hist, L.hist_words,
                           state, L.S);
        const size_t hw = (size_t)L.S * MT_BINS;
        hipLaunchKernelGGL(mt_hist_kernel<0>, grid, dim3(MT_THREADS), 0, st, a, hist, state);
        hipLaunchKernelGGL(mt_select_kernel<0>, dim3(L.S), dim3(MT_THREADS), 0, st, hist, state, a.eigen);
        hipLaunchKernelGGL(mt_hist_kernel<1>, grid, dim3(MT_THREADS), 0, st, a, hist + hw, state);
        hipLaunchKernelGGL(mt_select_kernel<1>, dim3(L.S), dim3(MT_THREADS), 0, st, hist + hw, state, a.eigen);
        hipLaunchKernelGGL(mt_hist_kernel<2>, grid, dim3(MT_THREADS), 0, st, a, hist + 2 * hw, state);
        hipLaunchKernelGGL(mt_select_kernel<2>, dim3(L.S), dim3(MT_THREADS), 0, st, hist + 2 * hw, state, a.eigen);
        if (a.eigen) hipLaunchKernelGGL(mt_upper_kernel, grid, dim3(MT_THREADS), 0, st, a, state);
    }
    hipLaunchKernelGGL(mt_metrics_kernel, grid, dim3(MT_THREADS), 0, st, a, state, part);
    hipLaunchKernelGGL(mt_finalize_kernel, dim3(L.G), dim3(MT_THREADS), 0, st, a, state, part, out, d->ratios, d->status);
    DC_CHECK_LAUNCH();
    return DC_OK;
}
