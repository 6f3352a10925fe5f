// Joins of the coarse-to-fine ConvGRU front-end, gru_version v10 (reference networks/rnn.py:472-569 `ConvGRUBlocks_v9` with
// attention=False, :101-143 `ConvGRUCell`, :739-779 `FeatureFusionBlock_v2`, :783-791 `UpscalePS`; trainer_gru.py:716-764
// `run_gru_v9_v10`, evaluate_depth_gru_fusion_my_v.py:641-701 `evaluate_v9_v10_seq`).  The cell's two convolutions are fused
// conv blocks and r * h is dc_gru_rh / dc_gru_infer_rh; what is left of a frame at one scale is the GRU's tail and the block's
// hand-over, ONE launch here where v5's and v8's parts would take two (dc_gru_blend_* and dc_lstm_handover_*):
//   h_new = (1 - u) * h_prev + u * cnm          u = gates[:, C:2C]   (gates (B, 2C, h, w) = [reset | update], post-sigmoid)
//   pre   = relu(a + (h_prev + h_new) / 2)      a = resConfUnit1(input_1)
//   up    = PixelShuffle(2)(tanh(pre))          up[b, q, 2y + i, 2x + j] = tanh(pre[b, 4q + 2i + j, y, x])
// The item walk is the hand-over's (c2f_dev.h: four channels 4q..4q+3 at four neighbouring pixels per thread where C % 4 == 0,
// w % 4 == 0 and the bases are 16-byte aligned; one element per thread otherwise) with the GRU's tail as its cell, and the
// per-element expressions are those of gru.hip's blend and lstm_dev.h's hand-over, in their order.  The backward recomputes u and
// the tanh from what the forward read or wrote: per frame only gates, h_prev, cnm and pre are kept.  Every thread owns what it
// writes: no atomics, two runs give the same bits; no allocation or synchronisation: capturable.  tanh is the accurate tanhf: the
// state is carried over the frames.
#include "c2f_dev.h"

namespace dc {

__device__ __forceinline__ float gru_blend1(float u, float h, float cnm) { return (1.f - u) * h + u * cnm; }      // rnn.py:136
__device__ __forceinline__ float4 gru_blend1(float4 u, float4 h, float4 c) {
    return make_float4(gru_blend1(u.x, h.x, c.x), gru_blend1(u.y, h.y, c.y), gru_blend1(u.z, h.z, c.z), gru_blend1(u.w, h.w, c.w));
}

// ---- forward: training (h_new out of place) and the inference step (h_prev == h_new == h, in place) ---------------------------
// The cell: per element u (the update half of gates, b * 2CP + CP + ...), h_prev and cnm are read and h_new is written.
struct GruTailCell {
    const float *gates, *h_prev, *cnm;
    float* h_new;
    size_t CP;
    template <class V> struct S { V hp, hn; };
    template <class V> __device__ __forceinline__ S<V> eval(unsigned b, size_t o) const {
        const V hp = ld<V>(h_prev + o);
        return {hp, gru_blend1(ld<V>(gates + (size_t)b * CP + CP + o), hp, ld<V>(cnm + o))};
    }
    template <class V> __device__ __forceinline__ void store(size_t o, const S<V>& s) const { st(h_new + o, s.hn); }
};

// VEC: per channel of an item four float4 loads (u, h_prev, cnm, a) and two float4 stores (h_new, pre); up may be NULL
template <bool VEC>
__global__ __launch_bounds__(LSTM_BLOCK) void gru_handover_fwd_kernel(const float* __restrict__ gates, const float* __restrict__ h_prev,
                                                                     const float* __restrict__ cnm, const float* __restrict__ a,
                                                                     float* __restrict__ h_new, float* __restrict__ pre,
                                                                     float* __restrict__ up, unsigned n, int C, int h, int w) {
    const size_t CP = (size_t)C * h * w;
    handover_fwd_walk<VEC, false>(GruTailCell{gates, h_prev, cnm, h_new, CP}, a, nullptr, pre, up, CP, n, C, h, w);
}
// B lockstep windows, the state rewritten in place: h is read and written through the same pointer (each element by the thread
// that read it), so it is not __restrict__.  y (with r), pre and up may be NULL: the state update alone.
template <bool VEC>
__global__ __launch_bounds__(LSTM_BLOCK) void gru_c2f_infer_step_kernel(const float* __restrict__ gates, const float* __restrict__ cnm,
                                                                       const float* __restrict__ y, const float* __restrict__ r, float* h,
                                                                       float* pre, float* up, size_t up_bstride, unsigned n, int C, int hh,
                                                                       int w) {
    handover_fwd_walk<VEC, true>(GruTailCell{gates, h, cnm, h, (size_t)C * hh * w}, y, r, pre, up, up_bstride, n, C, hh, w);
}

// ---- training backward -----------------------------------------------------------------------------------------------------
//   d = (pre > 0) * (g_pre + unshuffle(g_up) * (1 - tanh(pre)^2));   G = g_h_new + d / 2
//   d_a = d;  d_cnm = G * u;  d_gates = [0 | G * (cnm - h_prev)];  d_h_prev = d / 2 + G * (1 - u)
template <class V> struct C2fBwd { V da, dcnm, du, dh; };
__device__ __forceinline__ C2fBwd<float> gru_handover_bwd1(float u, float hp, float cn, float pre, float gh, float gp, float gu) {
    C2fBwd<float> r;
    r.da = handover_d(pre, gp, gu);
    const float half = r.da * 0.5f, G = gh + half;
    r.dcnm = G * u;
    r.du = G * (cn - hp);
    r.dh = half + G * (1.f - u);
    return r;
}
__device__ __forceinline__ C2fBwd<float4> gru_handover_bwd1(float4 u, float4 hp, float4 cn, float4 pre, float4 gh, float4 gp, float4 gu) {
    const C2fBwd<float> b0 = gru_handover_bwd1(u.x, hp.x, cn.x, pre.x, gh.x, gp.x, gu.x);
    const C2fBwd<float> b1 = gru_handover_bwd1(u.y, hp.y, cn.y, pre.y, gh.y, gp.y, gu.y);
    const C2fBwd<float> b2 = gru_handover_bwd1(u.z, hp.z, cn.z, pre.z, gh.z, gp.z, gu.z);
    const C2fBwd<float> b3 = gru_handover_bwd1(u.w, hp.w, cn.w, pre.w, gh.w, gp.w, gu.w);
    return {make_float4(b0.da, b1.da, b2.da, b3.da), make_float4(b0.dcnm, b1.dcnm, b2.dcnm, b3.dcnm),
            make_float4(b0.du, b1.du, b2.du, b3.du), make_float4(b0.dh, b1.dh, b2.dh, b3.dh)};
}
struct GruTailCellBwd {
    const float *gates, *h_prev, *cnm, *g_h_new;                                 // g_h_new may be NULL (zero)
    float *d_gates, *d_h_prev, *d_cnm, *d_a;
    size_t CP;
    template <class V> __device__ __forceinline__ void bwd(unsigned b, size_t o, V pre, V gp, V gu) const {
        const size_t go = (size_t)b * CP + o;                                    // reset half of the gates; update: + CP
        const C2fBwd<V> r = gru_handover_bwd1(ld<V>(gates + go + CP), ld<V>(h_prev + o), ld<V>(cnm + o), pre,
                                              g_h_new ? ld<V>(g_h_new + o) : V(), gp, gu);
        st(d_a + o, r.da);
        st(d_cnm + o, r.dcnm);
        st(d_h_prev + o, r.dh);
        st(d_gates + go, V());
        st(d_gates + go + CP, r.du);
    }
};
// g_h_new / g_pre / g_up may be NULL (zero)
template <bool VEC>
__global__ __launch_bounds__(LSTM_BLOCK) void gru_handover_bwd_kernel(const float* __restrict__ gates, const float* __restrict__ h_prev,
                                                                     const float* __restrict__ cnm, const float* __restrict__ pre,
                                                                     const float* __restrict__ g_h_new, const float* __restrict__ g_pre,
                                                                     const float* __restrict__ g_up, float* __restrict__ d_gates,
                                                                     float* __restrict__ d_h_prev, float* __restrict__ d_cnm,
                                                                     float* __restrict__ d_a, unsigned n, int C, int h, int w) {
    handover_bwd_walk<VEC>(GruTailCellBwd{gates, h_prev, cnm, g_h_new, d_gates, d_h_prev, d_cnm, d_a, (size_t)C * h * w}, pre, g_pre, g_up,
                           n, C, h, w);
}

}  // namespace dc

using namespace dc;

// every entry: sizes > 0 and gates, the largest tensor (2 B C h w), below 2^31 elements
extern "C" int dc_gru_handover_fwd(const float* gates, const float* h_prev, const float* cnm, const float* a, float* h_new, float* pre,
                                   float* up, int B, int C, int h, int w, void* stream) {
    size_t n;
    if (!gates || !h_prev || !cnm || !a || !h_new || !pre || !c2f_sizes(B, C, h, w, 2, &n)) return DC_EINVAL;
    if (up && (C & 3)) return DC_EINVAL;
    const bool vec = c2f_vec(C, w, up, (size_t)C * h * w, {gates, h_prev, cnm, a, h_new, pre, up});
    const C2fLaunch l = c2f_launch(vec, n);
    hipLaunchKernelGGL(vec ? gru_handover_fwd_kernel<true> : gru_handover_fwd_kernel<false>, dim3(l.grid), dim3(LSTM_BLOCK), 0,
                       (hipStream_t)stream, gates, h_prev, cnm, a, h_new, pre, up, l.count, C, h, w);
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" int dc_gru_handover_bwd(const float* gates, const float* h_prev, const float* cnm, const float* pre, const float* g_h_new,
                                   const float* g_pre, const float* g_up, float* d_gates, float* d_h_prev, float* d_cnm, float* d_a, int B,
                                   int C, int h, int w, void* stream) {
    size_t n;
    if (!gates || !h_prev || !cnm || !pre || !d_gates || !d_h_prev || !d_cnm || !d_a || !c2f_sizes(B, C, h, w, 2, &n)) return DC_EINVAL;
    if ((!g_h_new && !g_pre && !g_up) || (g_up && (C & 3))) return DC_EINVAL;
    const bool vec = c2f_vec(C, w, nullptr, 0, {gates, h_prev, cnm, pre, g_h_new, g_pre, g_up, d_gates, d_h_prev, d_cnm, d_a});
    const C2fLaunch l = c2f_launch(vec, n);
    hipLaunchKernelGGL(vec ? gru_handover_bwd_kernel<true> : gru_handover_bwd_kernel<false>, dim3(l.grid), dim3(LSTM_BLOCK), 0,
                       (hipStream_t)stream, gates, h_prev, cnm, pre, g_h_new, g_pre, g_up, d_gates, d_h_prev, d_cnm, d_a, l.count, C, h, w);
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" int dc_gru_c2f_infer_step(const float* gates, const float* cnm, const float* y, const float* r, float* h, float* pre, float* up,
                                     size_t up_bstride, int B, int C, int hh, int w, void* stream) {
    size_t n;
    if (!gates || !cnm || !h || !c2f_sizes(B, C, hh, w, 2, &n)) return DC_EINVAL;
    if ((y == nullptr) != (r == nullptr) || ((pre || up) && !y)) return DC_EINVAL;
    if (up && ((C & 3) || up_bstride < (size_t)C * hh * w)) return DC_EINVAL;
    const bool vec = c2f_vec(C, w, up, up_bstride, {gates, cnm, y, r, h, pre, up});
    const C2fLaunch l = c2f_launch(vec, n);
    hipLaunchKernelGGL(vec ? gru_c2f_infer_step_kernel<true> : gru_c2f_infer_step_kernel<false>, dim3(l.grid), dim3(LSTM_BLOCK), 0,
                       (hipStream_t)stream, gates, cnm, y, r, h, pre, up, up_bstride, l.count, C, hh, w);
    DC_CHECK_LAUNCH();
    return DC_OK;
}
