// The coarse-to-fine hand-over's item walk, stated once for its six entries: dc_lstm_handover_fwd / _bwd (lstm.hip),
// dc_lstm_infer_step (lstm_infer.hip) and dc_gru_handover_fwd / _bwd, dc_gru_c2f_infer_step (gru_c2f.hip).
//   pre = relu(a + (h_prev + h_new) / 2),   up[b, q, 2y + i, 2x + j] = tanh(pre[b, 4q + 2i + j, y, x])      (PixelShuffle(2))
// float4 form: an item is the four channels 4q..4q+3 at four neighbouring pixels of a row, items = B * (C/4) * h * (w/4); the
// item's 16 values of tanh(pre) leave as two output rows of eight pixels.  Scalar form: one element per thread, n = B * C * h * w.
// A file supplies its CELL -- where (h_prev, h_new) of an element come from and what state is stored -- and the walk does the
// rest: the decode, `a` or `y + r`, pre, up, the incoming gradients and every NULL case.  A cell's members are the kernel's own
// arguments, so what is __restrict__ there stays so here; the walks' pointers are qualified by their callers alone.
//   forward cell    template <class V> S<V> eval(unsigned b, size_t o) const     S<V>: at least { V hp, hn; }
//                   template <class V> void store(size_t o, const S<V>&) const   (after pre was written: a state may be in place)
//   backward cell   template <class V> void bwd(unsigned b, size_t o, V pre, V g_pre, V g_up) const
// V is float or float4, b the batch item and o the element's (first element's) index in a (B, C, h, w) tensor.
// Launch shape: LSTM_BLOCK threads, lstm_grid blocks, a grid-stride loop, one launch; every thread owns what it writes.
#pragma once
#include "lstm_dev.h"

namespace dc {

// ---- float and float4 under one name ---------------------------------------------------------------------------------------
template <class V> __device__ __forceinline__ V ld(const float* p) { return *reinterpret_cast<const V*>(p); }
template <class V> __device__ __forceinline__ void st(float* p, V v) { *reinterpret_cast<V*>(p) = v; }

__device__ __forceinline__ float add2(float a, float b) { return a + b; }
__device__ __forceinline__ float4 add2(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float halve(float v) { return v * 0.5f; }
__device__ __forceinline__ float4 halve(float4 v) { return make_float4(v.x * 0.5f, v.y * 0.5f, v.z * 0.5f, v.w * 0.5f); }
__device__ __forceinline__ float4 handover_pre(float4 a, float4 hp, float4 hn) {
    return make_float4(handover_pre(a.x, hp.x, hn.x), handover_pre(a.y, hp.y, hn.y), handover_pre(a.z, hp.z, hn.z),
                       handover_pre(a.w, hp.w, hn.w));
}
__device__ __forceinline__ float4 handover_d(float4 pre, float4 gp, float4 gu) {
    return make_float4(handover_d(pre.x, gp.x, gu.x), handover_d(pre.y, gp.y, gu.y), handover_d(pre.z, gp.z, gu.z),
                       handover_d(pre.w, gp.w, gu.w));
}

// ---- where an item or an element lives ---------------------------------------------------------------------------------------
// b: batch item; in0: element (b, 4q, y, 4 x4) of a (B, C, h, w) tensor, the item's channel k is k * h * w further on;
// up0: element (q, 2y, 8 x4) of the batch item's (C/4, 2h, 2w) block of up -- its rows may be strided: add b * up_bstride
struct C2fItem { unsigned b; size_t in0, up0; };
__device__ __forceinline__ C2fItem c2f_item(unsigned it, int C, int h, int w) {
    const unsigned w4 = w >> 2, C4 = C >> 2, P = (unsigned)h * w;
    const unsigned x4 = it % w4, t = it / w4, y = t % h, bq = t / h, q = bq % C4;
    C2fItem m;
    m.b = bq / C4;
    m.in0 = (size_t)m.b * C * P + (size_t)q * 4 * P + (size_t)y * w + 4 * x4;
    m.up0 = (size_t)q * 4 * P + (size_t)(2 * y) * (2 * w) + 8 * x4;
    return m;
}
// the same block's position of element rem = (channel ch, pixel (y, x)) of a batch item
__device__ __forceinline__ size_t shuffled(unsigned rem, int h, int w) {
    const unsigned P = (unsigned)h * w, x = rem % w, t = rem / w, y = t % h, ch = t / h, k = ch & 3, q = ch >> 2;
    return (size_t)q * 4 * P + (size_t)(2 * y + (k >> 1)) * (2 * w) + 2 * x + (k & 1);
}
// tanh of the item's pre (p[k]: channel 4q + k, pixels x..x+3) as its two rows of eight pixels at u0, and the way back
__device__ __forceinline__ void shuffle_store(float* u0, const float4 (&p)[4], int w) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float4 e = p[2 * i], o = p[2 * i + 1];                             // j = 0 / 1
        float* row = u0 + (size_t)i * 2 * w;
        st(row, make_float4(tanhf(e.x), tanhf(o.x), tanhf(e.y), tanhf(o.y)));
        st(row + 4, make_float4(tanhf(e.z), tanhf(o.z), tanhf(e.w), tanhf(o.w)));
    }
}
__device__ __forceinline__ void shuffle_gather(const float* u0, float4 (&g)[4], int w) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float* row = u0 + (size_t)i * 2 * w;
        const float4 lo = ld<float4>(row), hi = ld<float4>(row + 4);
        g[2 * i] = make_float4(lo.x, lo.z, hi.x, hi.z);
        g[2 * i + 1] = make_float4(lo.y, lo.w, hi.y, hi.w);
    }
}

// ---- the forward walk ----------------------------------------------------------------------------------------------------------
// pre of one element / four pixels of a channel.  STEP (the inference steps): a = y + r, and y (with r) or pre may be NULL.
template <bool STEP, class V, class Cell>
__device__ __forceinline__ V handover_at(const Cell& cell, unsigned b, size_t o, const float* a, const float* r, float* pre) {
    const auto s = cell.template eval<V>(b, o);
    V p = V();
    if (!STEP || a) {
        p = handover_pre(STEP ? add2(ld<V>(a + o), ld<V>(r + o)) : ld<V>(a + o), s.hp, s.hn);
        if (!STEP || pre) st(pre + o, p);
    }
    cell.template store<V>(o, s);
    return p;
}
// n: items (VEC) or elements; up may be NULL (with STEP it is given only with y); up_bstride: C * h * w where up is contiguous
template <bool VEC, bool STEP, class Cell>
__device__ __forceinline__ void handover_fwd_walk(const Cell& cell, const float* a, const float* r, float* pre, float* up,
                                                  size_t up_bstride, unsigned n, int C, int h, int w) {
    const unsigned P = (unsigned)h * w, CP = (unsigned)C * P;
    for (unsigned it = blockIdx.x * LSTM_BLOCK + threadIdx.x; it < n; it += gridDim.x * LSTM_BLOCK) {
        if constexpr (VEC) {
            const C2fItem m = c2f_item(it, C, h, w);
            float4 p[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) p[k] = handover_at<STEP, float4>(cell, m.b, m.in0 + (size_t)k * P, a, r, pre);
            if (up) shuffle_store(up + (size_t)m.b * up_bstride + m.up0, p, w);
        } else {
            const unsigned b = it / CP;
            const float v = handover_at<STEP, float>(cell, b, it, a, r, pre);
            if (up) up[(size_t)b * up_bstride + shuffled(it - b * CP, h, w)] = tanhf(v);
        }
    }
}

// ---- the backward walk ---------------------------------------------------------------------------------------------------------
// g_pre / g_up may be NULL (zero); the cell forms d(pre pre-ReLU) with handover_d and stores what its entry returns
template <bool VEC, class Cell>
__device__ __forceinline__ void handover_bwd_walk(const Cell& cell, const float* pre, const float* g_pre, const float* g_up, unsigned n,
                                                  int C, int h, int w) {
    const unsigned P = (unsigned)h * w, CP = (unsigned)C * P;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (unsigned it = blockIdx.x * LSTM_BLOCK + threadIdx.x; it < n; it += gridDim.x * LSTM_BLOCK) {
        if constexpr (VEC) {
            const C2fItem m = c2f_item(it, C, h, w);
            float4 gu[4] = {zero, zero, zero, zero};                              // per channel k, pixels x..x+3
            if (g_up) shuffle_gather(g_up + (size_t)m.b * CP + m.up0, gu, w);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const size_t o = m.in0 + (size_t)k * P;
                cell.template bwd<float4>(m.b, o, ld<float4>(pre + o), g_pre ? ld<float4>(g_pre + o) : zero, gu[k]);
            }
        } else {
            const unsigned b = it / CP;
            const float gu = g_up ? g_up[(size_t)b * CP + shuffled(it - b * CP, h, w)] : 0.f;
            cell.template bwd<float>(b, it, pre[it], g_pre ? g_pre[it] : 0.f, gu);
        }
    }
}

// ---- what the entries share ------------------------------------------------------------------------------------------------------
// sizes > 0 and the call's largest tensor, mult * n elements with n = B C h w, below 2^31
static inline bool c2f_sizes(int B, int C, int h, int w, int mult, size_t* n) {
    if (B <= 0 || C <= 0 || h <= 0 || w <= 0) return false;
    *n = (size_t)B * C * h * w;
    return *n * mult < (1ull << 31);
}
// the float4 form: whole channel quads, whole pixel quads, rows of up a multiple of 4 floats apart, every base 16-byte aligned
static inline bool c2f_vec(int C, int w, const void* up, size_t up_bstride, std::initializer_list<const void*> ps) {
    return (C & 3) == 0 && (w & 3) == 0 && (!up || (up_bstride & 3) == 0) && all16(ps);
}
struct C2fLaunch { unsigned grid, count; };                                       // count: n / 16 items or n elements
static inline C2fLaunch c2f_launch(bool vec, size_t n) {
    const size_t work = vec ? n >> 4 : n;
    return {lstm_grid(work), (unsigned)work};
}

}  // namespace dc
