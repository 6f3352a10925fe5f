// Image panels of the training log (the reference's trainer.py:666-698 writes the frames, the warped predictions, the normalised
// disparities and the automask of up to four items): every item's pictures are composed into ONE interleaved uint8 panel on the
// device, so that a log step moves bytes to the host and not some twenty float tensors per item.
// include/depthcore.h: dc_log_panel.
//
// A panel is described by tiles (dc_panel_tile): a source plane (or three), a nearest-neighbour factor and a corner.  At most
// three launches on the caller's stream:
//   clear    every byte of the panels to `background` (whole dwords between a byte head and tail: the buffer may start at any
//            address), and every NORM tile's range keys to (all ones, zero);
//   range    NORM tiles only (skipped when there is none): the exact minimum and maximum of the tile's h*w source values by
//            32-bit integer atomicMin / atomicMax of order-preserving keys (render.hip's rd_key) -- integer min / max commute,
//            there is no floating-point atomic, two calls give the same bytes;
//   compose  one thread per run of four destination pixels of a tile row: 12 bytes, stored as three dwords when the run is
//            whole and its address dword aligned (every run of the trainer's layout is), byte by byte otherwise -- a panel row
//            is 3*PW bytes and a tile starts at byte 3*x0, so neither is aligned in general.  The colour table sits in LDS as
//            256 packed words.
// The tiles of a call do not overlap (checked on the host), so no byte is written by two threads of the compose pass.
// Built with -ffp-contract=off: `v * 255.0f + 0.5f` is a rounded product and a rounded sum, as numpy forms it.
#include <algorithm>

#include "dc_common.h"

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_RUN = 4;                  // destination pixels per thread: 12 bytes = 3 dwords
constexpr int LP_MAX_Y = 1024;             // blocks along y (a block strides over what is left)

// order-preserving map of fp32 onto uint32 and back (render.hip: rd_key / rd_val)
__device__ __forceinline__ unsigned lp_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float lp_val(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// RGB / UNIT: v <= 0 or NaN -> 0, v >= 1 -> 255, else (uint8)(v * 255.0f + 0.5f) in fp32
__device__ __forceinline__ unsigned lp_byte(float v) {
    if (!(v > 0.f)) return 0u;
    if (v >= 1.f) return 255u;
    return (unsigned)(uint8_t)(v * 255.0f + 0.5f);
}

__global__ __launch_bounds__(LP_THREADS) void lp_clear_kernel(uint8_t* panels, size_t nbytes, unsigned bg, unsigned* keys, int n_tiles) {
    const size_t stride = (size_t)gridDim.x * LP_THREADS, t0 = (size_t)blockIdx.x * LP_THREADS + threadIdx.x;
    const size_t to_dword = (size_t)(-(intptr_t)panels) & 3u, head = to_dword < nbytes ? to_dword : nbytes;
    const size_t words = (nbytes - head) / 4, tail0 = head + words * 4;
    unsigned* body = reinterpret_cast<unsigned*>(panels + head);
    const unsigned word = bg * 0x01010101u;
    for (size_t i = t0; i < words; i += stride) body[i] = word;
    if (t0 < head) panels[t0] = (uint8_t)bg;
    if (t0 < nbytes - tail0) panels[tail0 + t0] = (uint8_t)bg;
    for (size_t i = t0; i < (size_t)n_tiles; i += stride) {
        keys[2 * i] = 0xffffffffu;
        keys[2 * i + 1] = 0u;
    }
}

// grid (n_tiles, blocks per tile)
__global__ __launch_bounds__(LP_THREADS) void lp_range_kernel(const dc_panel_tile* __restrict__ tiles, unsigned* __restrict__ keys) {
    const dc_panel_tile t = tiles[blockIdx.x];
    if (t.kind != DC_TILE_NORM) return;
    const float* src = static_cast<const float*>(t.src);
    const long long n = (long long)t.h * t.w;
    unsigned lo = 0xffffffffu, hi = 0u;
    for (long long i = (long long)blockIdx.y * LP_THREADS + threadIdx.x; i < n; i += (long long)gridDim.y * LP_THREADS) {
        const unsigned k = lp_key(src[i]);
        lo = min(lo, k);
        hi = max(hi, k);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, (unsigned)__shfl_xor((int)lo, o));
        hi = max(hi, (unsigned)__shfl_xor((int)hi, o));
    }
    if ((threadIdx.x & 63) == 0 && lo <= hi) {                 // (a wave that saw no element holds lo > hi)
        atomicMin(&keys[2 * (size_t)blockIdx.x], lo);
        atomicMax(&keys[2 * (size_t)blockIdx.x + 1], hi);
    }
}

// grid (n_tiles, blocks per tile).  Packed colour: r | g << 8 | b << 16.
__global__ __launch_bounds__(LP_THREADS) void lp_compose_kernel(const dc_panel_tile* __restrict__ tiles, const unsigned* __restrict__ keys,
                                                                const uint8_t* __restrict__ lut, uint8_t* __restrict__ panels, int PH,
                                                                int PW) {
    __shared__ unsigned pal[256];
    const dc_panel_tile t = tiles[blockIdx.x];
    if (t.kind == DC_TILE_NORM)
        for (int i = threadIdx.x; i < 256; i += LP_THREADS)
            pal[i] = (unsigned)lut[3 * i] | ((unsigned)lut[3 * i + 1] << 8) | ((unsigned)lut[3 * i + 2] << 16);
    __syncthreads();
    float mi = 0.f, d = 1.f;
    if (t.kind == DC_TILE_NORM) {                              // normalize_image (utils.py): ma != mi ? ma - mi : 1e5
        mi = lp_val(keys[2 * (size_t)blockIdx.x]);
        const float ma = lp_val(keys[2 * (size_t)blockIdx.x + 1]);
        d = ma != mi ? ma - mi : 1e5f;
    }
    const int tw = t.w * t.up, th = t.h * t.up;
    const int rpr = (tw + LP_RUN - 1) / LP_RUN;                // runs per tile row
    const long long runs = (long long)th * rpr;
    const size_t plane = (size_t)t.h * t.w;
    const float* sf = static_cast<const float*>(t.src);
    const uint8_t* sb = static_cast<const uint8_t*>(t.src);
    for (long long r = (long long)blockIdx.y * LP_THREADS + threadIdx.x; r < runs; r += (long long)gridDim.y * LP_THREADS) {
        const int y = (int)(r / rpr), x = (int)(r - (long long)y * rpr) * LP_RUN;
        const int cnt = min(LP_RUN, tw - x);
        const size_t row = (size_t)(y / t.up) * t.w;
        unsigned c[LP_RUN] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < LP_RUN; ++k) {
            if (k >= cnt) break;
            const size_t s = row + (size_t)((x + k) / t.up);
            if (t.kind == DC_TILE_RGB) {
                c[k] = lp_byte(sf[s]) | (lp_byte(sf[plane + s]) << 8) | (lp_byte(sf[2 * plane + s]) << 16);
            } else if (t.kind == DC_TILE_UNIT) {
                c[k] = lp_byte(sf[s]) * 0x010101u;
            } else if (t.kind == DC_TILE_MASK) {
                c[k] = (int)sb[s] >= t.thr ? 0xffffffu : 0u;
            } else {
                const float xn = (sf[s] - mi) / d;
                const float xa = xn * 256.0f;
                c[k] = pal[xa < 0.f ? 0 : min((int)xa, 255)];
            }
        }
        uint8_t* o = panels + (((size_t)t.panel * PH + t.y0 + y) * PW + t.x0 + x) * 3;
        if (cnt == LP_RUN && ((uintptr_t)o & 3u) == 0) {
            unsigned* w = reinterpret_cast<unsigned*>(o);
            w[0] = c[0] | (c[1] << 24);
            w[1] = (c[1] >> 8) | (c[2] << 16);
            w[2] = (c[2] >> 16) | (c[3] << 8);
        } else {                                               // the end of a tile row, or a run at an odd address
            for (int k = 0; k < cnt; ++k) {
                o[3 * k] = (uint8_t)(c[k] & 0xffu);
                o[3 * k + 1] = (uint8_t)((c[k] >> 8) & 0xffu);
                o[3 * k + 2] = (uint8_t)(c[k] >> 16);
            }
        }
    }
}

// every refusal of the header comment; no HIP call.  max_src / max_dst: the largest h*w of a NORM tile (0: none) and the
// largest count of destination runs of a tile.
bool lp_check(const dc_panel_tile* tiles, int n_tiles, int n_panels, int PH, int PW, long long& max_src, long long& max_runs) {
    max_src = max_runs = 0;
    for (int i = 0; i < n_tiles; ++i) {
        const dc_panel_tile& t = tiles[i];
        if (!t.src || t.kind < DC_TILE_RGB || t.kind > DC_TILE_MASK || t.up < 1 || t.h < 1 || t.w < 1) return false;
        if (t.panel < 0 || t.panel >= n_panels || t.x0 < 0 || t.y0 < 0) return false;
        const long long tw = (long long)t.w * t.up, th = (long long)t.h * t.up;
        if (t.x0 + tw > PW || t.y0 + th > PH) return false;                  // (so tw, th fit an int)
        const long long hw = (long long)t.h * t.w;
        if (hw >= 0x7fffffffLL || t.src_elems < (t.kind == DC_TILE_RGB ? 3 * hw : hw)) return false;
        if (t.kind != DC_TILE_MASK && ((uintptr_t)t.src & 3u)) return false;
        if (t.kind == DC_TILE_NORM) max_src = std::max(max_src, hw);
        max_runs = std::max(max_runs, th * ((tw + LP_RUN - 1) / LP_RUN));
        for (int j = 0; j < i; ++j) {
            const dc_panel_tile& u = tiles[j];
            if (u.panel != t.panel) continue;
            const long long uw = (long long)u.w * u.up, uh = (long long)u.h * u.up;
            if (t.x0 < u.x0 + uw && u.x0 < t.x0 + tw && t.y0 < u.y0 + uh && u.y0 < t.y0 + th) return false;
        }
    }
    return true;
}

unsigned lp_blocks(long long work) { return (unsigned)std::min<long long>((work + LP_THREADS - 1) / LP_THREADS, LP_MAX_Y); }

}  // namespace

extern "C" size_t dc_log_panel_ws_bytes(int n_tiles) { return n_tiles < 1 ? 0 : (size_t)n_tiles * 2 * sizeof(unsigned); }

extern "C" int dc_log_panel(const dc_panel_tile* tiles_host, const dc_panel_tile* tiles_dev, int n_tiles, const uint8_t* lut,
                            uint8_t* panels, int n_panels, int PH, int PW, int background, void* ws, size_t ws_bytes, void* stream) {
    if (n_tiles < 1 || n_panels < 1 || n_panels > 65535 || PH < 1 || PW < 1 || !tiles_host || !tiles_dev || !lut || !panels ||
        background < 0 || background > 255)
        return DC_EINVAL;
    long long max_src, max_runs;
    if (!lp_check(tiles_host, n_tiles, n_panels, PH, PW, max_src, max_runs)) return DC_EINVAL;
    if (ws_bytes < dc_log_panel_ws_bytes(n_tiles)) return DC_EWORKSPACE;
    if (!ws || ((uintptr_t)ws & 3u)) return DC_EINVAL;
    const size_t nbytes = (size_t)n_panels * PH * PW * 3;
    unsigned* keys = static_cast<unsigned*>(ws);
    const hipStream_t st = (hipStream_t)stream;
    const size_t clear_work = std::max<size_t>(nbytes / 4 + 4, (size_t)n_tiles);
    hipLaunchKernelGGL(lp_clear_kernel, dim3((unsigned)std::min<size_t>((clear_work + LP_THREADS - 1) / LP_THREADS, 8192)), dim3(LP_THREADS),
                       0, st, panels, nbytes, (unsigned)background, keys, n_tiles);
    if (max_src > 0)
        hipLaunchKernelGGL(lp_range_kernel, dim3(n_tiles, lp_blocks((max_src + 7) / 8)), dim3(LP_THREADS), 0, st, tiles_dev, keys);
    hipLaunchKernelGGL(lp_compose_kernel, dim3(n_tiles, lp_blocks(max_runs)), dim3(LP_THREADS), 0, st, tiles_dev, (const unsigned*)keys, lut,
                       panels, PH, PW);
    DC_CHECK_LAUNCH();
    return DC_OK;
}
