// Colour rendering of a disparity map, the reference's test_simple.py:126-145: the decoder's disparity upsampled to the photo's
// size, vmin = min, vmax = np.percentile(., q), matplotlib's Normalize and a 256-entry colour table -> RGB bytes.
// include/depthcore.h: dc_disp_render.
//
// The upsampled map is never stored: every pass re-derives a pixel with bilinear_at (the expression of
// dc_upsample_bilinear_fwd) from the low-resolution map, which stays in L2 (480 KB per 192 x 640 image), as metrics.hip does.
// Grid (blocks per image, N) for the selection passes; every image has its own range.
//   zero                histograms, selection state
//   hist(0) select(0)   12-bit digit (key bits 31..20) of every pixel's key -> the digit holding rank lo = floor((n-1) q/100);
//                       the smallest key of the image (vmin) by integer atomicMin on the way
//   hist(1) select(1)   the next 12 bits (19..8) among the keys with that prefix
//   hist(2) select(2)   the last 8 bits, and the smallest key above the 24-bit prefix (integer atomicMin): s[lo] exactly, and
//                       s[lo+1] -- the same key when the run of equal keys reaches rank lo+1, else the next occupied bin of the
//                       last histogram, else the smallest key above the prefix.  numpy's _lerp of the two in fp64 -> range
//   colour              a run of four pixels per thread over the flat (image, pixel) index: three whole dwords per store,
//                       whatever the image size; the table sits in LDS as 256 packed words
// One range for a whole drive (dc_disp_range_pooled, dc_disp_render_fixed): the same passes over the values of all N images as
// ONE population -- one histogram, one selection state, rank floor((N n - 1) q/100), one select block -- which write a single
// (vmin, vmax) pair; the colour pass alone then renders any number of images against a pair read from device memory.
// Histograms and minima are integer atomics (order-independent), there is no floating-point atomic: two calls give the same
// bytes.  No fast-math; the percentile interpolation and the normalisation are compiled with `fp contract(off)` at function
// scope (as eval.hip's numpy expressions), so their fp64 products, sums and the division and the fp32 roundings are the stated
// ones.  The file itself keeps the library's default contraction: bilinear_at has to compile here to the bits it has in
// dc_upsample_bilinear_fwd and metrics.hip, and a file-wide -ffp-contract=off would unfuse its multiply-adds.
#include "dc_common.h"

namespace dc {

constexpr int RD_THREADS = 256;
constexpr int RD_PPT = 8;                              // pixels per thread per block of the selection passes
constexpr int RD_TILE = RD_THREADS * RD_PPT;
constexpr int RD_BINS = 4096;
constexpr int RD_RUN = 4;                              // pixels per thread of the colour pass: 12 bytes = 3 dwords
constexpr int RD_MAX_BLOCKS = 8192;

struct RdState {                                       // one per image
    unsigned rank, prefix, key_min, min_above;
};

struct RdArgs {
    const float* disp;
    int N, h, w, Ho, Wo, n, nbx;
    unsigned lo;                                       // rank floor((n-1) q/100)
    int hi_same;                                       // min(lo+1, n-1) == lo
    double g;                                          // (n-1) q/100 - lo
    float ry, rx;
};

// order-preserving map of fp32 onto uint32 (metrics.hip: mt_key / mt_val)
__device__ __forceinline__ unsigned rd_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float rd_val(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ float rd_pixel(const RdArgs& a, int b, int j) {
    const int oy = j / a.Wo, ox = j - oy * a.Wo;
    return bilinear_at(a.disp + (size_t)b * a.h * a.w, a.h, a.w, a.Ho, a.Wo, oy, ox, a.ry, a.rx);
}

__global__ __launch_bounds__(256) void rd_zero_kernel(unsigned* p, size_t n, RdState* st, int S) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = 0u;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < S; s += (int)stride) {
        RdState z;
        z.rank = 0u;
        z.prefix = 0u;
        z.key_min = 0xffffffffu;
        z.min_above = 0xffffffffu;
        st[s] = z;
    }
}

__device__ __forceinline__ unsigned rd_wave_min(unsigned m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = min(m, (unsigned)__shfl_xor((int)m, o));
    return m;
}

// pass 0: bin = key >> 20, and the image's smallest key;  pass 1: (key >> 8) & 0xfff of keys whose top 12 bits are the selected
// prefix;  pass 2: key & 0xff of keys whose top 24 bits are, and the smallest key above that prefix.
// POOLED (dc_disp_range_pooled): the N images are ONE population -- one histogram and one selection state for all of them
// (slot 0, not indexed by image), and a block walks the tiles blockIdx.x, blockIdx.x + gridDim.x, .. of its image, so that a
// long drive reaches the shared histogram with a bounded number of blocks; its bins stay private in LDS until the walk ends.
template <int PASS, bool POOLED = false>
__global__ __launch_bounds__(RD_THREADS) void rd_hist_kernel(RdArgs a, unsigned* __restrict__ hist, RdState* __restrict__ st) {
    __shared__ unsigned sh[RD_BINS];
    constexpr int NB = PASS == 2 ? 256 : RD_BINS;
    const int b = blockIdx.y, slot = POOLED ? 0 : b;
    for (int i = threadIdx.x; i < NB; i += RD_THREADS) sh[i] = 0u;
    const unsigned pre = PASS > 0 ? st[slot].prefix : 0u;
    __syncthreads();
    unsigned m = 0xffffffffu;
    int tile = blockIdx.x;                                         // < a.nbx: the grid's x extent is at most nbx
    do {
        const int j0 = tile * RD_TILE;
        for (int k = 0; k < RD_PPT; ++k) {
            const int j = j0 + k * RD_THREADS + threadIdx.x;
            if (j >= a.n) continue;
            const unsigned key = rd_key(rd_pixel(a, b, j));
            if (PASS == 0) {
                atomicAdd(&sh[key >> 20], 1u);
                m = min(m, key);
            } else if (PASS == 1) {
                if ((key >> 20) == pre) atomicAdd(&sh[(key >> 8) & 0xfffu], 1u);
            } else {
                if ((key >> 8) == pre) atomicAdd(&sh[key & 0xffu], 1u);
                else if ((key >> 8) > pre) m = min(m, key);
            }
        }
        tile += gridDim.x;
    } while (POOLED && tile < a.nbx);
    if (PASS != 1) {
        m = rd_wave_min(m);
        if ((threadIdx.x & 63) == 0 && m != 0xffffffffu) atomicMin(PASS == 0 ? &st[slot].key_min : &st[slot].min_above, m);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NB; i += RD_THREADS) {
        const unsigned c = sh[i];
        if (c) atomicAdd(&hist[(size_t)slot * RD_BINS + i], c);
    }
}

// numpy's _lerp (lib/_function_base_impl.py) of a = s[lo], b = s[hi] at g: diff in the array's type, the products in fp64
__device__ __forceinline__ float rd_lerp(float a, float b, double g) {
#pragma clang fp contract(off)
    const float diff = b - a;
    const double v = g < 0.5 ? (double)a + (double)diff * g : (double)b - (double)diff * (1.0 - g);
    return (float)v;
}

// one block per image: the bin holding the image's rank.  Integer arithmetic throughout; the last pass writes the range.
template <int PASS>
__global__ __launch_bounds__(RD_THREADS) void rd_select_kernel(RdArgs a, const unsigned* __restrict__ hist, RdState* __restrict__ st,
                                                               float* __restrict__ range) {
    __shared__ unsigned wsum[RD_THREADS / 64];
    constexpr int NB = PASS == 2 ? 256 : RD_BINS, PER = NB / RD_THREADS;
    const int s = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const unsigned* h = hist + (size_t)s * RD_BINS;
    RdState m = st[s];
    unsigned c[PER], tot = 0u;
#pragma unroll
    for (int i = 0; i < PER; ++i) { c[i] = h[t * PER + i]; tot += c[i]; }
    unsigned inc = tot;                                            // inclusive scan: wave scan, then the wave totals
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    unsigned before = inc - tot;
    for (int i = 0; i < wv; ++i) before += wsum[i];
    const unsigned r = PASS == 0 ? a.lo : m.rank;                  // the rank among the keys that share the prefix so far
    if (r < before || r >= before + tot) return;                   // exactly one thread owns it
    unsigned cum = before;
    int bin = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        if (r < cum + c[i]) { bin = t * PER + i; break; }
        cum += c[i];
    }
    m.rank = r - cum;
    if (PASS == 0) m.prefix = (unsigned)bin;
    else if (PASS == 1) m.prefix = (m.prefix << 12) | (unsigned)bin;
    st[s] = m;
    if (PASS != 2) return;
    const unsigned key_lo = (m.prefix << 8) | (unsigned)bin;
    unsigned key_hi = key_lo;
    if (!a.hi_same && m.rank + 1u >= h[bin]) {                     // rank lo + 1 lies beyond the run of keys equal to s[lo]
        key_hi = m.min_above;                                      // exists: lo + 1 <= n - 1
        for (int i = bin + 1; i < 256; ++i)
            if (h[i]) { key_hi = (m.prefix << 8) | (unsigned)i; break; }
    }
    range[2 * s] = rd_val(m.key_min);
    range[2 * s + 1] = rd_lerp(rd_val(key_lo), rd_val(key_hi), a.g);
}

// matplotlib's Normalize (process_value's fp32 array, the in-place `-= vmin`, `/= vmax - vmin` with fp64 scalars) and
// Colormap.__call__ (xa *= N; truncation; "over" = the last colour) -> table index
__device__ __forceinline__ int rd_index(float d, float vmin, float vmax, double den) {
#pragma clang fp contract(off)
    if (vmin == vmax) return 0;
    float x = (float)((double)d - (double)vmin);
    x = (float)((double)x / den);
    const float xa = x * 256.0f;
    return xa < 0.f ? 0 : (xa >= 256.f ? 255 : (int)xa);
}

// run r covers pixels 4r .. 4r+3 of the flat (image, pixel) index, bytes 12r .. 12r+11 of rgb: dword aligned for any Ho x Wo.
// A run may cross into the next image, whose range is then loaded.  FIXED (dc_disp_render_fixed): range holds ONE pair, shared
// by all images.
template <bool FIXED = false>
__global__ __launch_bounds__(RD_THREADS) void rd_colour_kernel(RdArgs a, const uint8_t* __restrict__ lut, const float* __restrict__ range,
                                                               uint8_t* __restrict__ rgb) {
    __shared__ unsigned pal[256];
    for (int i = threadIdx.x; i < 256; i += RD_THREADS)
        pal[i] = (unsigned)lut[3 * i] | ((unsigned)lut[3 * i + 1] << 8) | ((unsigned)lut[3 * i + 2] << 16);
    __syncthreads();
    const size_t total = (size_t)a.N * a.n, runs = (total + RD_RUN - 1) / RD_RUN;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < runs; r += stride) {
        const size_t p0 = r * RD_RUN;
        int img = (int)(p0 / (size_t)a.n);
        int pos = (int)(p0 - (size_t)img * a.n);
        float vmin = range[FIXED ? 0 : 2 * img], vmax = range[FIXED ? 1 : 2 * img + 1];
        double den = (double)vmax - (double)vmin;
        const int cnt = (int)min((size_t)RD_RUN, total - p0);
        unsigned c[RD_RUN] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < RD_RUN; ++k) {
            if (k >= cnt) break;
            if (pos == a.n) {
                ++img;
                pos = 0;
                if (!FIXED) {
                    vmin = range[2 * img];
                    vmax = range[2 * img + 1];
                    den = (double)vmax - (double)vmin;
                }
            }
            c[k] = pal[rd_index(rd_pixel(a, img, pos), vmin, vmax, den)];
            ++pos;
        }
        if (cnt == RD_RUN) {
            unsigned* o = reinterpret_cast<unsigned*>(rgb + p0 * 3);
            o[0] = c[0] | (c[1] << 24);
            o[1] = (c[1] >> 8) | (c[2] << 16);
            o[2] = (c[2] >> 16) | (c[3] << 8);
        } else {                                                   // the last, partial run of the whole output
            for (int k = 0; k < cnt; ++k) {
                uint8_t* o = rgb + (p0 + k) * 3;
                o[0] = (uint8_t)(c[k] & 0xffu);
                o[1] = (uint8_t)((c[k] >> 8) & 0xffu);
                o[2] = (uint8_t)(c[k] >> 16);
            }
        }
    }
}

struct RdLayout {
    size_t hist_words, state_off, bytes;
};

static bool rd_layout(int N, int h, int w, int Ho, int Wo, RdArgs& a, RdLayout& L) {
    if (N < 1 || N > 65535 || h < 1 || w < 1 || Ho < 1 || Wo < 1) return false;          // N is the grid's y extent
    const long long n = (long long)Ho * Wo;
    if (n >= 0x7fffffffLL - RD_TILE || (long long)h * w >= 0x7fffffffLL) return false;
    a.N = N; a.h = h; a.w = w; a.Ho = Ho; a.Wo = Wo;
    a.n = (int)n;
    a.nbx = (int)((n + RD_TILE - 1) / RD_TILE);
    a.ry = (float)h / (float)Ho;                               // as dc_upsample_bilinear_fwd
    a.rx = (float)w / (float)Wo;
    L.hist_words = (size_t)3 * N * RD_BINS;
    L.state_off = L.hist_words * sizeof(unsigned);
    L.bytes = L.state_off + (size_t)N * sizeof(RdState);
    return true;
}

// numpy's virtual index (n - 1) * (q / 100) in fp64, its floor and the fraction, for a population of n values
static void rd_rank(RdArgs& a, unsigned long long n, double q) {
    const double vi = (double)(n - 1) * (q / 100.0);
    double lo = floor(vi);
    if (lo > (double)(n - 1)) lo = (double)(n - 1);
    a.lo = (unsigned)lo;
    a.hi_same = (unsigned long long)a.lo + 1u > n - 1;
    a.g = vi - lo;
}

constexpr int RD_POOL_BLOCKS = 2048;                   // blocks that reach the one pooled histogram, about (ceil: at most N more)

// the pooled population: the same per-image limits, and N * Ho * Wo < 2^32 -- ranks and bin counts are 32-bit
static bool rd_pool_layout(int N, int h, int w, int Ho, int Wo, RdArgs& a, RdLayout& L) {
    if (!rd_layout(N, h, w, Ho, Wo, a, L)) return false;
    if ((unsigned long long)N * (unsigned long long)a.n >= (1ull << 32)) return false;
    L.hist_words = (size_t)3 * RD_BINS;
    L.state_off = L.hist_words * sizeof(unsigned);
    L.bytes = L.state_off + sizeof(RdState);
    return true;
}

}  // namespace dc

using namespace dc;

extern "C" size_t dc_disp_render_ws_bytes(int N, int h, int w, int Ho, int Wo) {
    RdArgs a;
    RdLayout L;
    return rd_layout(N, h, w, Ho, Wo, a, L) ? L.bytes : 0;
}

extern "C" int dc_disp_render(const float* disp, const uint8_t* lut, uint8_t* rgb, float* range, int N, int h, int w, int Ho, int Wo,
                              double q, void* ws, size_t ws_bytes, void* stream) {
    RdArgs a;
    RdLayout L;
    if (!rd_layout(N, h, w, Ho, Wo, a, L) || !disp || !lut || !rgb || !range || !ws || !(q >= 0.0 && q <= 100.0) ||
        ((uintptr_t)rgb & 3u))                                 // the colour pass stores whole dwords
        return DC_EINVAL;
    if (ws_bytes < L.bytes) return DC_EWORKSPACE;
    a.disp = disp;
    rd_rank(a, (unsigned long long)a.n, q);                    // the same for every image of the call
    hipStream_t st = (hipStream_t)stream;
    unsigned* hist = (unsigned*)ws;
    RdState* state = (RdState*)((char*)ws + L.state_off);
    const size_t hw = (size_t)N * RD_BINS;
    const dim3 grid(a.nbx, N);
    hipLaunchKernelGGL(rd_zero_kernel, dim3(std::min((int)((L.hist_words + 255) / 256), 1024)), dim3(256), 0, st, hist, L.hist_words, state, N);
    hipLaunchKernelGGL(rd_hist_kernel<0>, grid, dim3(RD_THREADS), 0, st, a, hist, state);
    hipLaunchKernelGGL(rd_select_kernel<0>, dim3(N), dim3(RD_THREADS), 0, st, a, hist, state, range);
    hipLaunchKernelGGL(rd_hist_kernel<1>, grid, dim3(RD_THREADS), 0, st, a, hist + hw, state);
    hipLaunchKernelGGL(rd_select_kernel<1>, dim3(N), dim3(RD_THREADS), 0, st, a, hist + hw, state, range);
    hipLaunchKernelGGL(rd_hist_kernel<2>, grid, dim3(RD_THREADS), 0, st, a, hist + 2 * hw, state);
    hipLaunchKernelGGL(rd_select_kernel<2>, dim3(N), dim3(RD_THREADS), 0, st, a, hist + 2 * hw, state, range);
    const size_t runs = ((size_t)N * a.n + RD_RUN - 1) / RD_RUN;
    const int blocks = (int)std::min<size_t>((runs + RD_THREADS - 1) / RD_THREADS, RD_MAX_BLOCKS);
    hipLaunchKernelGGL(rd_colour_kernel<false>, dim3(blocks), dim3(RD_THREADS), 0, st, a, lut, range, rgb);
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" size_t dc_disp_range_pooled_ws_bytes(int N, int h, int w, int Ho, int Wo) {
    RdArgs a;
    RdLayout L;
    return rd_pool_layout(N, h, w, Ho, Wo, a, L) ? L.bytes : 0;
}

extern "C" int dc_disp_range_pooled(const float* disp, float* range, int N, int h, int w, int Ho, int Wo, double q, void* ws,
                                    size_t ws_bytes, void* stream) {
    RdArgs a;
    RdLayout L;
    if (!rd_pool_layout(N, h, w, Ho, Wo, a, L) || !disp || !range || !ws || !(q >= 0.0 && q <= 100.0)) return DC_EINVAL;
    if (ws_bytes < L.bytes) return DC_EWORKSPACE;
    a.disp = disp;
    rd_rank(a, (unsigned long long)N * (unsigned long long)a.n, q);
    hipStream_t st = (hipStream_t)stream;
    unsigned* hist = (unsigned*)ws;
    RdState* state = (RdState*)((char*)ws + L.state_off);
    const dim3 grid(std::min(a.nbx, (RD_POOL_BLOCKS + N - 1) / N), N);
    hipLaunchKernelGGL(rd_zero_kernel, dim3((int)((L.hist_words + 255) / 256)), dim3(256), 0, st, hist, L.hist_words, state, 1);
    hipLaunchKernelGGL((rd_hist_kernel<0, true>), grid, dim3(RD_THREADS), 0, st, a, hist, state);
    hipLaunchKernelGGL(rd_select_kernel<0>, dim3(1), dim3(RD_THREADS), 0, st, a, hist, state, range);
    hipLaunchKernelGGL((rd_hist_kernel<1, true>), grid, dim3(RD_THREADS), 0, st, a, hist + RD_BINS, state);
    hipLaunchKernelGGL(rd_select_kernel<1>, dim3(1), dim3(RD_THREADS), 0, st, a, hist + RD_BINS, state, range);
    hipLaunchKernelGGL((rd_hist_kernel<2, true>), grid, dim3(RD_THREADS), 0, st, a, hist + 2 * RD_BINS, state);
    hipLaunchKernelGGL(rd_select_kernel<2>, dim3(1), dim3(RD_THREADS), 0, st, a, hist + 2 * RD_BINS, state, range);
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" int dc_disp_render_fixed(const float* disp, const uint8_t* lut, const float* range, uint8_t* rgb, int N, int h, int w, int Ho,
                                    int Wo, void* stream) {
    RdArgs a;
    RdLayout L;
    if (!rd_layout(N, h, w, Ho, Wo, a, L) || !disp || !lut || !range || !rgb || ((uintptr_t)rgb & 3u)) return DC_EINVAL;
    a.disp = disp;
    const size_t runs = ((size_t)N * a.n + RD_RUN - 1) / RD_RUN;
    const int blocks = (int)std::min<size_t>((runs + RD_THREADS - 1) / RD_THREADS, RD_MAX_BLOCKS);
    hipLaunchKernelGGL(rd_colour_kernel<true>, dim3(blocks), dim3(RD_THREADS), 0, (hipStream_t)stream, a, lut, range, rgb);
    DC_CHECK_LAUNCH();
    return DC_OK;
}
