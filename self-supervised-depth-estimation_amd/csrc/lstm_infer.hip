// Inference form of a ConvLSTM v8 frame at one scale (reference evaluate_depth_gru_fusion.py:557-618 `evaluate_v8_seq` over
// networks/rnn.py:70-79, 767-773, 783-791), ONE launch where training takes dc_lstm_cell_fwd, the `+ r` of ResidualConvUnit
// and dc_lstm_handover_fwd:
//   c' = s(f) * c + s(i) * tanh(g),  h' = s(o) * tanh(c')                 cc (B, 4C, hh, w) = [i | f | o | g]
//   pre = relu((y + r) + (h + h') / 2),  up = PixelShuffle(2)(tanh(pre))  y: resConfUnit1.conv2's output, r: the unit's ReLU-ed input
//   h <- h',  c <- c'                                                     in place: no trace, no backward
// Nothing is kept for a backward.  A thread reads h and c of its elements before it writes them and no other thread touches
// them: no atomics, two runs give the same bits; no allocation or synchronisation: capturable.  h and c are read and written
// through the same pointer, so neither is __restrict__.  The expressions are lstm.hip's (lstm_dev.h), accurate expf / tanhf; the
// item walk is the hand-over's (c2f_dev.h) with the LSTM step as its cell.
#include "c2f_dev.h"

namespace dc {

// The cell: per element the four gate planes of cc (C * P floats apart), c and h; h' and c' go back where h and c were read.
struct LstmStepCell {
    const float* cc;
    float *h, *c;
    size_t CP;
    template <class V> struct S { V hp, hn, cn; };
    __device__ __forceinline__ S<float> step(float vi, float vf, float vo, float vg, float vc, float vh) const {
        const LstmFwd r = lstm_fwd1(vi, vf, vo, vg, vc);
        return {vh, r.h, r.c};
    }
    __device__ __forceinline__ S<float4> step(float4 vi, float4 vf, float4 vo, float4 vg, float4 vc, float4 vh) const {
        const LstmFwd r0 = lstm_fwd1(vi.x, vf.x, vo.x, vg.x, vc.x), r1 = lstm_fwd1(vi.y, vf.y, vo.y, vg.y, vc.y);
        const LstmFwd r2 = lstm_fwd1(vi.z, vf.z, vo.z, vg.z, vc.z), r3 = lstm_fwd1(vi.w, vf.w, vo.w, vg.w, vc.w);
        return {vh, make_float4(r0.h, r1.h, r2.h, r3.h), make_float4(r0.c, r1.c, r2.c, r3.c)};
    }
    template <class V> __device__ __forceinline__ S<V> eval(unsigned b, size_t o) const {
        const float* g = cc + (size_t)b * 3 * CP + o;                            // gate i of the element: b * 4 CP + (o - b * CP)
        return step(ld<V>(g), ld<V>(g + CP), ld<V>(g + 2 * CP), ld<V>(g + 3 * CP), ld<V>(c + o), ld<V>(h + o));
    }
    template <class V> __device__ __forceinline__ void store(size_t o, const S<V>& s) const {
        st(h + o, s.hn);
        st(c + o, s.cn);
    }
};

// VEC (C % 4 == 0, w % 4 == 0, 16-byte aligned bases, up_bstride % 4 == 0): per channel of an item 6 or, with y, 8 float4 loads
// and float4 stores of h, c and pre.  y (with r), pre and up may be NULL: the state update alone.
template <bool VEC>
__global__ __launch_bounds__(LSTM_BLOCK) void lstm_infer_step_kernel(const float* __restrict__ cc, const float* __restrict__ y,
                                                                    const float* __restrict__ r, float* h, float* c, float* pre,
                                                                    float* up, size_t up_bstride, unsigned n, int C, int hh, int w) {
    handover_fwd_walk<VEC, true>(LstmStepCell{cc, h, c, (size_t)C * hh * w}, y, r, pre, up, up_bstride, n, C, hh, w);
}

}  // namespace dc

using namespace dc;

extern "C" int dc_lstm_infer_step(const float* cc, const float* y, const float* r, float* h, float* c, float* pre, float* up,
                                  size_t up_bstride, int B, int C, int hh, int w, void* stream) {
    size_t n;                                                                    // cc is the largest tensor: 4 B C hh w elements
    if (!cc || !h || !c || !c2f_sizes(B, C, hh, w, 4, &n)) return DC_EINVAL;
    if ((y == nullptr) != (r == nullptr) || ((pre || up) && !y)) return DC_EINVAL;
    if (up && ((C & 3) || up_bstride < (size_t)C * hh * w)) return DC_EINVAL;
    const bool vec = c2f_vec(C, w, up, up_bstride, {cc, y, r, h, c, pre, up});
    const C2fLaunch l = c2f_launch(vec, n);
    hipLaunchKernelGGL(vec ? lstm_infer_step_kernel<true> : lstm_infer_step_kernel<false>, dim3(l.grid), dim3(LSTM_BLOCK), 0,
                       (hipStream_t)stream, cc, y, r, h, c, pre, up, up_bstride, l.count, C, hh, w);
    DC_CHECK_LAUNCH();
    return DC_OK;
}
