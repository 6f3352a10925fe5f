// 7x7 local self-attention of the attention encoder (reference networks/attention.py:29-52 = resnet_encoder_attention.py:43-66,
// built with kernel 7, padding 3, stride 1, bias=False at :150-153), the part behind the three 1x1 convolutions, forward and
// backward.  The reference materialises two (B,C,H,W,7,7) unfolds, the logits, the softmax and the einsum operand (1.15 GB each
// at layer 1 of the BASELINE shape); here q, k, v are read once and y written once.
//
//   logit_t[c] = q[c] * (k_t[c] + rel_t[c]),  rel_t = rel_h[c][dy] for c < C/2, rel_w[c - C/2][dx] otherwise;  t = (dy, dx) in 7x7
//   y[c] = sum_t softmax_t(logit)[c] * v_t[c];   lse[c] = logsumexp_t(logit)[c];   out-of-image taps carry k = v = 0 and stay in
//   the softmax.  `groups` of the reference has no effect: this is 49-tap attention per (b, c) channel plane.
//
// Geometry (sasa_plan, the same for both directions): the map is cut into balanced tiles of at most 16 x 32 pixels
// (tiles = ceil(H/16) x ceil(W/32), tile = ceil(H/tiles_y) x ceil(W/tiles_x)); a block of 256 threads takes `np` consecutive
// channel planes (flat index b*C + c) of one tile position, np = up to 768 pixels' worth, so that the 12 x 40 and 6 x 20 planes of
// the deep stages fill a block (3 and 6 planes) instead of leaving it mostly idle.  Work items (plane, pixel) are dealt to the
// threads round-robin: consecutive lanes hold consecutive pixels of a row, so the 49 LDS reads of a tap walk consecutive banks.
//
// Forward: k, v of the tile + 3-pixel ring in LDS; per pixel the 49 logits stay in registers, explicit maximum, exp2-based exp.
// Backward, two phases in one kernel.  First dk, dv are GATHERED: with p' = p + o_t the pixel tap t of p reads,
//   dv[p'] = sum_t a_t[p] gy[p],   dk[p'] = sum_t a_t[p] gy[p] (v[p'] - y[p]) q[p],   p = p' - o_t   (p inside the image)
// so q, lse, gy, y of the tile + ring go to LDS and each thread recomputes the weights a_t = exp(logit_t - lse) that point at its
// own pixel.  The second phase is forward-shaped (k, v ring in LDS): dl_t = a_t gy (v_t - y), dq and the rel sums.
// Rel gradients: per item 7 sums -> LDS -> 8 strided part sums per (plane, k) -> one partial row per (block, plane), every order
// fixed; a second kernel sums the rows of a channel over images and tiles, 64 at a time.  No atomics.
#include "dc_common.h"

namespace dc {

constexpr int SA_K = 7, SA_R = 3;                  // window, ring
constexpr int SA_TH = 16, SA_TW = 32;              // largest tile
constexpr int SA_ITEMS = 768;                      // work items of a block: at most three per thread
constexpr int SA_REGION = 1536;                    // floats of one staged array: np * (th + 6) * (tw + 6) <= SA_REGION
constexpr int SA_PARTS = 8;                        // strided part sums of the rel-gradient block reduction
constexpr int SA_MAXNP = SA_REGION / (SA_K * SA_K);

struct SasaPlan { int th, tw, tiles_x, tiles_y, np, nblocks; };

struct SasaArgs {
    const float *q, *k, *v;
    long long qs, ks, vs;       // batch strides, elements
    const float *rel_h, *rel_w;
    float *y, *lse;             // forward outputs (lse may be null)
    const float *yin, *lsein, *gy;
    float *dq, *dk, *dv, *partial;
    int C, H, W, BC;
    int th, tw, tiles_x, tiles_y, np;
};

struct SasaBlk {
    int plane0, ty0, tx0, rw, rsz, px, items;
    __device__ __forceinline__ SasaBlk(const SasaArgs& a) {
        const int tiles = a.tiles_x * a.tiles_y, bid = blockIdx.x;
        const int zb = bid / tiles, tile = bid - zb * tiles, tyi = tile / a.tiles_x;
        plane0 = zb * a.np; ty0 = tyi * a.th; tx0 = (tile - tyi * a.tiles_x) * a.tw;
        rw = a.tw + 2 * SA_R; rsz = (a.th + 2 * SA_R) * rw; px = a.th * a.tw; items = a.np * px;
    }
};

// one work item: plane `pl` of the block, tile pixel (ly, lx); `ok` when it is a pixel of the map
struct SasaItem {
    int pl, ly, lx, c;
    size_t off;                 // element offset in a plain (B,C,H,W) tensor
    size_t bc;                  // b, for the strided inputs
    bool ok;
    __device__ __forceinline__ SasaItem(const SasaArgs& a, const SasaBlk& g, int i) {
        pl = i / g.px;
        const int r = i - pl * g.px;
        ly = r / a.tw; lx = r - ly * a.tw;
        const int plane = g.plane0 + pl, py = g.ty0 + ly, pxx = g.tx0 + lx;
        ok = i < g.items && plane < a.BC && py < a.H && pxx < a.W;
        const int b = plane / a.C;
        c = plane - b * a.C;
        bc = (size_t)b;
        off = ((size_t)plane * a.H + py) * a.W + pxx;
    }
    // offset of the same element in an input with batch stride `bs`
    __device__ __forceinline__ size_t soff(const SasaArgs& a, long long bs) const {
        return bc * (size_t)bs + (off - bc * (size_t)a.C * a.H * a.W);
    }
};

// the 7 rel values of channel c: rel_h[c] (indexed by dy) for c < C/2, rel_w[c - C/2] (indexed by dx) otherwise
__device__ __forceinline__ void sasa_rel(const SasaArgs& a, int c, float (&rel)[SA_K], bool& is_h) {
    is_h = c < a.C / 2;
    const float* p = is_h ? a.rel_h + (size_t)c * SA_K : a.rel_w + (size_t)(c - a.C / 2) * SA_K;
#pragma unroll
    for (int i = 0; i < SA_K; ++i) rel[i] = p[i];
}

// stage NA arrays of the block's planes, tile + ring, into LDS (dst[j] + i); 0 outside the image / beyond the last plane
template <int NA>
__device__ __forceinline__ void sasa_stage(const SasaArgs& a, const SasaBlk& g, const float* const (&src)[NA], const long long (&bs)[NA],
                                           float* const (&dst)[NA]) {
    const size_t chw = (size_t)a.C * a.H * a.W;
    for (int i = threadIdx.x; i < a.np * g.rsz; i += 256) {
        const int pl = i / g.rsz, r = i - pl * g.rsz, ry = r / g.rw, rx = r - ry * g.rw;
        const int plane = g.plane0 + pl, py = g.ty0 - SA_R + ry, pxx = g.tx0 - SA_R + rx;
        const bool in = plane < a.BC && py >= 0 && py < a.H && pxx >= 0 && pxx < a.W;
        const int b = plane / a.C;
        const size_t inner = in ? ((size_t)plane * a.H + py) * a.W + pxx - (size_t)b * chw : 0;
#pragma unroll
        for (int j = 0; j < NA; ++j) dst[j][i] = in ? src[j][(size_t)b * (size_t)bs[j] + inner] : 0.f;
    }
}

// the rel value of tap (dy, dx): IS_H channels (c < C/2) index their 7 values by dy, the others by dx.  A template parameter, so
// that the select is resolved once per item (one branch, uniform in a wave unless it spans both halves) and not once per tap.
template <bool IS_H>
__device__ __forceinline__ float sasa_rel_at(const float (&rel)[SA_K], int dy, int dx) { return IS_H ? rel[dy] : rel[dx]; }

// =====================================================================================================================
// forward
// =====================================================================================================================
template <bool IS_H>
__device__ __forceinline__ void sasa_fwd_item(const SasaArgs& a, const SasaItem& it, const float (&rel)[SA_K], const float* kb,
                                              const float* vb, int rw) {
    const float q = a.q[it.soff(a, a.qs)];
    float lg[SA_K * SA_K];
    float m = -INFINITY;
#pragma unroll
    for (int dy = 0; dy < SA_K; ++dy)
#pragma unroll
        for (int dx = 0; dx < SA_K; ++dx) {
            const float kr = kb[dy * rw + dx] + sasa_rel_at<IS_H>(rel, dy, dx);
            lg[dy * SA_K + dx] = q * kr;
            m = fmaxf(m, lg[dy * SA_K + dx]);
        }
    float s = 0.f, o = 0.f;
#pragma unroll
    for (int dy = 0; dy < SA_K; ++dy)
#pragma unroll
        for (int dx = 0; dx < SA_K; ++dx) {
            const float e = __expf(lg[dy * SA_K + dx] - m);
            s += e;
            o = fmaf(e, vb[dy * rw + dx], o);
        }
    a.y[it.off] = o / s;
    if (a.lse) a.lse[it.off] = m + logf(s);
}

__global__ __launch_bounds__(256) void sasa_fwd_kernel(SasaArgs a) {
    __shared__ float sk[SA_REGION], sv[SA_REGION];
    const SasaBlk g(a);
    {
        const float* const src[2] = {a.k, a.v};
        const long long bs[2] = {a.ks, a.vs};
        float* const dst[2] = {sk, sv};
        sasa_stage<2>(a, g, src, bs, dst);
    }
    __syncthreads();
#pragma unroll 1
    for (int i = threadIdx.x; i < g.items; i += 256) {
        const SasaItem it(a, g, i);
        if (!it.ok) continue;
        float rel[SA_K];
        bool is_h;
        sasa_rel(a, it.c, rel, is_h);
        const int base = it.pl * g.rsz + it.ly * g.rw + it.lx;
        if (is_h) sasa_fwd_item<true>(a, it, rel, sk + base, sv + base, g.rw);
        else sasa_fwd_item<false>(a, it, rel, sk + base, sv + base, g.rw);
    }
}

// =====================================================================================================================
// backward
// =====================================================================================================================
// dk, dv of one pixel: tap (dy, dx) of the pixel at (ly + 3 - dy, lx + 3 - dx) lands here; qb points at region index
// (ly + 6, lx + 6) of the staged q, with lse, gy, y of the same pixel SA_REGION, 2 SA_REGION, 3 SA_REGION floats behind it
template <bool IS_H>
__device__ __forceinline__ void sasa_gather_item(const SasaArgs& a, const SasaItem& it, const float (&rel)[SA_K], const float* qb, int rw) {
    const float k = a.k[it.soff(a, a.ks)], v = a.v[it.soff(a, a.vs)];
    float dk = 0.f, dv = 0.f;
#pragma unroll
    for (int dy = 0; dy < SA_K; ++dy)
#pragma unroll
        for (int dx = 0; dx < SA_K; ++dx) {
            const float* e = qb - dy * rw - dx;
            const float qq = e[0];
            // a pixel outside the image was staged as q = lse = gy = y = 0: weight exp(0) = 1 times gy = 0
            const float w = __expf(fmaf(qq, k + sasa_rel_at<IS_H>(rel, dy, dx), -e[SA_REGION]));
            const float ag = w * e[2 * SA_REGION];
            dv += ag;
            dk = fmaf(ag * (v - e[3 * SA_REGION]), qq, dk);
        }
    a.dk[it.off] = dk;
    a.dv[it.off] = dv;
}

// dq of one pixel and its 7 rel sums (over dx for IS_H channels, over dy for the others) -> red[kk * items]
template <bool IS_H>
__device__ __forceinline__ void sasa_dq_item(const SasaArgs& a, const SasaItem& it, const float (&rel)[SA_K], const float* kb, int rw,
                                             float* red, int items) {
    const float q = a.q[it.soff(a, a.qs)], gy = a.gy[it.off], y = a.yin[it.off], lse = a.lsein[it.off];
    const float* vb = kb + SA_REGION;
    float sums[SA_K], dq = 0.f;
#pragma unroll
    for (int i = 0; i < SA_K; ++i) sums[i] = 0.f;
#pragma unroll
    for (int dy = 0; dy < SA_K; ++dy)
#pragma unroll
        for (int dx = 0; dx < SA_K; ++dx) {
            const float kr = kb[dy * rw + dx] + sasa_rel_at<IS_H>(rel, dy, dx);
            const float w = __expf(fmaf(q, kr, -lse));                 // a_t
            const float dl = w * gy * (vb[dy * rw + dx] - y);           // d logit_t
            dq = fmaf(dl, kr, dq);
            sums[IS_H ? dy : dx] += dl * q;
        }
    a.dq[it.off] = dq;
#pragma unroll
    for (int i = 0; i < SA_K; ++i) red[i * items] = sums[i];
}

constexpr int SA_RED = 2 * SA_REGION;                  // offset of the rel sums in the backward's LDS, behind the staged k, v

__global__ __launch_bounds__(256) void sasa_bwd_kernel(SasaArgs a) {
    // the gather stages q, lse, gy, y in [0, 4 SA_REGION); then k, v go to [0, 2 SA_REGION), the items' rel sums to [SA_RED, SA_RED
    // + 7 SA_ITEMS) and, once k and v are dead, their part sums to [0, SA_MAXNP * 7 * SA_PARTS)
    __shared__ float sm[SA_RED + SA_K * SA_ITEMS];
    static_assert(SA_RED + SA_K * SA_ITEMS >= 4 * SA_REGION && SA_MAXNP * SA_K * SA_PARTS <= SA_RED, "LDS layout of sasa_bwd_kernel");
    const SasaBlk g(a);
    // ---- dk, dv gathered from the pixels whose window reaches this one
    {
        const float* const src[4] = {a.q, a.lsein, a.gy, a.yin};
        const long long plain = (long long)a.C * a.H * a.W;
        const long long bs[4] = {a.qs, plain, plain, plain};
        float* const dst[4] = {sm, sm + SA_REGION, sm + 2 * SA_REGION, sm + 3 * SA_REGION};
        sasa_stage<4>(a, g, src, bs, dst);
    }
    __syncthreads();
#pragma unroll 1
    for (int i = threadIdx.x; i < g.items; i += 256) {
        const SasaItem it(a, g, i);
        if (!it.ok) continue;
        float rel[SA_K];
        bool is_h;
        sasa_rel(a, it.c, rel, is_h);
        const float* qb = sm + it.pl * g.rsz + (it.ly + 2 * SA_R) * g.rw + it.lx + 2 * SA_R;
        if (is_h) sasa_gather_item<true>(a, it, rel, qb, g.rw);
        else sasa_gather_item<false>(a, it, rel, qb, g.rw);
    }
    __syncthreads();
    // ---- dq and the rel sums (taps of the item's own pixel): forward-shaped, k and v of tile + ring in LDS
    {
        const float* const src[2] = {a.k, a.v};
        const long long bs[2] = {a.ks, a.vs};
        float* const dst[2] = {sm, sm + SA_REGION};
        sasa_stage<2>(a, g, src, bs, dst);
    }
    __syncthreads();
    float* red = sm + SA_RED;
#pragma unroll 1
    for (int i = threadIdx.x; i < g.items; i += 256) {
        const SasaItem it(a, g, i);
        if (!it.ok) {                                  // every item slot is written: the part sums below read them all
#pragma unroll
            for (int kk = 0; kk < SA_K; ++kk) red[kk * g.items + i] = 0.f;
            continue;
        }
        float rel[SA_K];
        bool is_h;
        sasa_rel(a, it.c, rel, is_h);
        const float* kb = sm + it.pl * g.rsz + it.ly * g.rw + it.lx;
        if (is_h) sasa_dq_item<true>(a, it, rel, kb, g.rw, red + i, g.items);
        else sasa_dq_item<false>(a, it, rel, kb, g.rw, red + i, g.items);
    }
    __syncthreads();
    // ---- rel partial rows: LDS [k][item] -> SA_PARTS strided sums per (plane, k) -> the row, all in fixed order
    float* part = sm;
    for (int j = threadIdx.x; j < a.np * SA_K * SA_PARTS; j += 256) {
        const int pl = j / (SA_K * SA_PARTS), r = j - pl * (SA_K * SA_PARTS), kk = r / SA_PARTS, p = r - kk * SA_PARTS;
        const float* row = red + kk * g.items + pl * g.px;
        float s = 0.f;
        for (int e = p; e < g.px; e += SA_PARTS) s += row[e];
        part[j] = s;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < a.np * SA_K; j += 256) {
        float s = 0.f;
#pragma unroll
        for (int p = 0; p < SA_PARTS; ++p) s += part[j * SA_PARTS + p];
        a.partial[(size_t)blockIdx.x * a.np * SA_K + j] = s;           // row (block, plane), planes beyond the last: 0
    }
}

// sum of the partial rows of one (channel, k) entry over images and tiles: one wave per entry, 64 rows per pass, fixed order
__global__ __launch_bounds__(64) void sasa_rel_reduce_kernel(const float* __restrict__ partial, float* __restrict__ drel_h,
                                                            float* __restrict__ drel_w, int B, int C, int tiles, int np) {
    const int c = blockIdx.x / SA_K, kk = blockIdx.x - c * SA_K;
    float s = 0.f;
    for (int n = threadIdx.x; n < B * tiles; n += 64) {
        const int b = n / tiles, tile = n - b * tiles;
        const int plane = b * C + c, zb = plane / np, pl = plane - zb * np;
        s += partial[(((size_t)zb * tiles + tile) * np + pl) * SA_K + kk];
    }
    s = wave_sum(s);
    if (threadIdx.x == 0) {
        if (c < C / 2) drel_h[c * SA_K + kk] = s;
        else drel_w[(c - C / 2) * SA_K + kk] = s;
    }
}

}  // namespace dc

using namespace dc;

static bool sasa_plan(int B, int C, int H, int W, SasaPlan& p) {
    if (B <= 0 || C < 2 || (C & 1) || H <= 0 || W <= 0) return false;
    unsigned long long n = (unsigned long long)B * (unsigned long long)C;
    if (n >= (1ull << 31)) return false;
    n *= (unsigned long long)H;
    if (n >= (1ull << 31)) return false;
    n *= (unsigned long long)W;
    if (n >= (1ull << 31)) return false;
    p.tiles_x = ceil_div(W, SA_TW); p.tw = ceil_div(W, p.tiles_x);
    p.tiles_y = ceil_div(H, SA_TH); p.th = ceil_div(H, p.tiles_y);
    int np = SA_ITEMS / (p.th * p.tw);
    np = np < 1 ? 1 : np;
    const int fit = SA_REGION / ((p.th + 2 * SA_R) * (p.tw + 2 * SA_R));
    np = np > fit ? fit : np;
    np = np > B * C ? B * C : np;
    p.np = np;
    p.nblocks = p.tiles_x * p.tiles_y * ceil_div(B * C, np);      // < 2^31: every block but the ragged ones owns >= 1 element
    return true;
}

static bool sasa_args(SasaArgs& a, SasaPlan& p, const float* q, const float* k, const float* v, long long qs, long long ks, long long vs,
                      const float* rel_h, const float* rel_w, int B, int C, int H, int W) {
    if (!q || !k || !v || !rel_h || !rel_w || !sasa_plan(B, C, H, W, p)) return false;
    const long long chw = (long long)C * H * W;
    if (qs < chw || ks < chw || vs < chw) return false;
    a = SasaArgs{};
    a.q = q; a.k = k; a.v = v; a.qs = qs; a.ks = ks; a.vs = vs; a.rel_h = rel_h; a.rel_w = rel_w;
    a.C = C; a.H = H; a.W = W; a.BC = B * C;
    a.th = p.th; a.tw = p.tw; a.tiles_x = p.tiles_x; a.tiles_y = p.tiles_y; a.np = p.np;
    return true;
}

extern "C" int dc_sasa_plan(int B, int C, int H, int W, int* plan) {
    SasaPlan p;
    if (!plan || !sasa_plan(B, C, H, W, p)) return DC_EINVAL;
    plan[0] = p.th; plan[1] = p.tw; plan[2] = p.tiles_x; plan[3] = p.tiles_y; plan[4] = p.np;
    return DC_OK;
}

extern "C" int dc_sasa_fwd(const float* q, const float* k, const float* v, long long q_bstride, long long k_bstride, long long v_bstride,
                           const float* rel_h, const float* rel_w, float* y, float* lse, int B, int C, int H, int W, void* stream) {
    SasaArgs a;
    SasaPlan p;
    if (!y || !sasa_args(a, p, q, k, v, q_bstride, k_bstride, v_bstride, rel_h, rel_w, B, C, H, W)) return DC_EINVAL;
    a.y = y; a.lse = lse;
    hipLaunchKernelGGL(sasa_fwd_kernel, dim3(p.nblocks), dim3(256), 0, (hipStream_t)stream, a);
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" size_t dc_sasa_bwd_workspace(int B, int C, int H, int W) {
    SasaPlan p;
    if (!sasa_plan(B, C, H, W, p)) return 0;
    return (size_t)p.nblocks * p.np * SA_K * sizeof(float);
}

extern "C" int dc_sasa_bwd(const float* q, const float* k, const float* v, long long q_bstride, long long k_bstride, long long v_bstride,
                           const float* rel_h, const float* rel_w, const float* y, const float* lse, const float* gy, float* dq,
                           float* dk, float* dv, float* drel_h, float* drel_w, void* ws, int B, int C, int H, int W, void* stream) {
    SasaArgs a;
    SasaPlan p;
    if (!y || !lse || !gy || !dq || !dk || !dv || !drel_h || !drel_w || !ws ||
        !sasa_args(a, p, q, k, v, q_bstride, k_bstride, v_bstride, rel_h, rel_w, B, C, H, W))
        return DC_EINVAL;
    a.yin = y; a.lsein = lse; a.gy = gy; a.dq = dq; a.dk = dk; a.dv = dv; a.partial = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sasa_bwd_kernel, dim3(p.nblocks), dim3(256), 0, st, a);
    DC_CHECK_LAUNCH();
    hipLaunchKernelGGL(sasa_rel_reduce_kernel, dim3(C * SA_K), dim3(64), 0, st, (const float*)ws, drel_h, drel_w, B, C,
                       p.tiles_x * p.tiles_y, p.np);
    DC_CHECK_LAUNCH();
    return DC_OK;
}
