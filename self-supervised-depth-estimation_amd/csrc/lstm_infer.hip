// Inference form of a ConvLSTM v8 frame at one scale (reference evaluate_depth_gru_fusion.py:557-618 `evaluate_v8_seq` over
// networks/rnn.py:70-79, 767-773, 783-791), ONE launch where training takes dc_lstm_cell_fwd, the `+ r` of ResidualConvUnit
// and dc_lstm_handover_fwd:
//   c' = s(f) * c + s(i) * tanh(g),  h' = s(o) * tanh(c')                 cc (B, 4C, hh, w) = [i | f | o | g]
//   pre = relu((y + r) + (h + h') / 2),  up = PixelShuffle(2)(tanh(pre))  y: resConfUnit1.conv2's output, r: the unit's ReLU-ed input
//   h <- h',  c <- c'                                                     in place: no trace, no backward
// Nothing is kept for a backward.  A thread reads h and c of its elements before it writes them and no other thread touches
// them: no atomics, two runs give the same bits; no allocation or synchronisation: capturable.  h and c are read and written
// through the same pointer, so neither is __restrict__.  The expressions are lstm.hip's (lstm_dev.h), accurate expf / tanhf.
#include "lstm_dev.h"

namespace dc {

// Vector form (C % 4 == 0, w % 4 == 0, 16-byte aligned bases, up_bstride % 4 == 0): lstm_handover_fwd_vec_kernel's item, the
// four channels 4q..4q+3 at four neighbouring pixels of a row.  Per channel: the four gate planes of cc (C * P floats apart,
// a multiple of 4 here), c, h and, with y, y and r -- 6 or 8 float4 loads -- and float4 stores of h, c and pre; the item's 16
// values of tanh(pre) leave as two output rows of eight pixels.   items = B * (C/4) * hh * (w/4)
__global__ __launch_bounds__(LSTM_BLOCK) void lstm_infer_step_vec_kernel(const float* __restrict__ cc, const float* __restrict__ y,
                                                                        const float* __restrict__ r, float* h, float* c, float* pre,
                                                                        float* up, size_t up_bstride, unsigned items, int C, int hh,
                                                                        int w) {
    const unsigned w4 = w >> 2, P = (unsigned)hh * w, C4 = C >> 2;
    const size_t CP = (size_t)C * P;
    for (unsigned it = blockIdx.x * LSTM_BLOCK + threadIdx.x; it < items; it += gridDim.x * LSTM_BLOCK) {
        const unsigned x4 = it % w4, t = it / w4, yy = t % hh, bq = t / hh, q = bq % C4, b = bq / C4;
        const size_t pix = (size_t)yy * w + 4 * x4;
        const size_t in0 = (size_t)b * CP + (size_t)q * 4 * P + pix;            // element of h / c / y / r / pre, channel 4q
        const float* g0 = cc + (size_t)b * 4 * CP + (size_t)q * 4 * P + pix;     // gate i of channel 4q
        float4 p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const size_t o = in0 + (size_t)k * P;
            const float* g = g0 + (size_t)k * P;
            const float4 vi = *reinterpret_cast<const float4*>(g), vf = *reinterpret_cast<const float4*>(g + CP);
            const float4 vo = *reinterpret_cast<const float4*>(g + 2 * CP), vg = *reinterpret_cast<const float4*>(g + 3 * CP);
            const float4 vc = *reinterpret_cast<const float4*>(c + o), vh = *reinterpret_cast<const float4*>(h + o);
            const LstmFwd r0 = lstm_fwd1(vi.x, vf.x, vo.x, vg.x, vc.x), r1 = lstm_fwd1(vi.y, vf.y, vo.y, vg.y, vc.y);
            const LstmFwd r2 = lstm_fwd1(vi.z, vf.z, vo.z, vg.z, vc.z), r3 = lstm_fwd1(vi.w, vf.w, vo.w, vg.w, vc.w);
            if (y) {
                const float4 vy = *reinterpret_cast<const float4*>(y + o), vr = *reinterpret_cast<const float4*>(r + o);
                p[k] = make_float4(handover_pre(vy.x + vr.x, vh.x, r0.h), handover_pre(vy.y + vr.y, vh.y, r1.h),
                                   handover_pre(vy.z + vr.z, vh.z, r2.h), handover_pre(vy.w + vr.w, vh.w, r3.h));
                if (pre) *reinterpret_cast<float4*>(pre + o) = p[k];
            }
            *reinterpret_cast<float4*>(h + o) = make_float4(r0.h, r1.h, r2.h, r3.h);
            *reinterpret_cast<float4*>(c + o) = make_float4(r0.c, r1.c, r2.c, r3.c);
        }
        if (up) {                                                                // (given only with y)
            float* u0 = up + (size_t)b * up_bstride + (size_t)q * 4 * P + (size_t)(2 * yy) * (2 * w) + 8 * x4;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float4 e = p[2 * i], o = p[2 * i + 1];                     // j = 0 / 1
                float* row = u0 + (size_t)i * 2 * w;
                *reinterpret_cast<float4*>(row) = make_float4(tanhf(e.x), tanhf(o.x), tanhf(e.y), tanhf(o.y));
                *reinterpret_cast<float4*>(row + 4) = make_float4(tanhf(e.z), tanhf(o.z), tanhf(e.w), tanhf(o.w));
            }
        }
    }
}

// Scalar form: one element of the state per thread; n = B * C * P
__global__ __launch_bounds__(LSTM_BLOCK) void lstm_infer_step_kernel(const float* __restrict__ cc, const float* __restrict__ y,
                                                                    const float* __restrict__ r, float* h, float* c, float* pre,
                                                                    float* up, size_t up_bstride, unsigned n, int C, int hh, int w) {
    const unsigned P = (unsigned)hh * w, CP = (unsigned)C * P;
    for (unsigned e = blockIdx.x * LSTM_BLOCK + threadIdx.x; e < n; e += gridDim.x * LSTM_BLOCK) {
        const unsigned b = e / CP, rem = e - b * CP;
        const float* g = cc + (size_t)b * 4 * CP + rem;
        const float h_cur = h[e];
        const LstmFwd s = lstm_fwd1(g[0], g[CP], g[2 * (size_t)CP], g[3 * (size_t)CP], c[e]);
        if (y) {
            const float v = handover_pre(y[e] + r[e], h_cur, s.h);
            if (pre) pre[e] = v;
            if (up) {
                const unsigned x = rem % w, t = rem / w, yy = t % hh, ch = t / hh, k = ch & 3, q = ch >> 2;
                up[(size_t)b * up_bstride + (size_t)q * 4 * P + (size_t)(2 * yy + (k >> 1)) * (2 * w) + 2 * x + (k & 1)] = tanhf(v);
            }
        }
        h[e] = s.h;
        c[e] = s.c;
    }
}

}  // namespace dc

using namespace dc;

extern "C" int dc_lstm_infer_step(const float* cc, const float* y, const float* r, float* h, float* c, float* pre, float* up,
                                  size_t up_bstride, int B, int C, int hh, int w, void* stream) {
    if (B <= 0 || C <= 0 || hh <= 0 || w <= 0 || !cc || !h || !c) return DC_EINVAL;
    if ((y == nullptr) != (r == nullptr) || ((pre || up) && !y)) return DC_EINVAL;
    const size_t n = (size_t)B * C * hh * w;
    if (n * 4 >= (1ull << 31)) return DC_EINVAL;                                 // cc is the largest tensor: 4 B C hh w elements
    if (up && ((C & 3) || up_bstride < (size_t)C * hh * w)) return DC_EINVAL;
    if ((C & 3) == 0 && (w & 3) == 0 && (!up || (up_bstride & 3) == 0) && all16({cc, y, r, h, c, pre, up})) {
        const size_t items = n >> 4;
        hipLaunchKernelGGL(lstm_infer_step_vec_kernel, dim3(lstm_grid(items)), dim3(LSTM_BLOCK), 0, (hipStream_t)stream, cc, y, r, h, c,
                           pre, up, up_bstride, (unsigned)items, C, hh, w);
    } else {
        hipLaunchKernelGGL(lstm_infer_step_kernel, dim3(lstm_grid(n)), dim3(LSTM_BLOCK), 0, (hipStream_t)stream, cc, y, r, h, c, pre, up,
                           up_bstride, (unsigned)n, C, hh, w);
    }
    DC_CHECK_LAUNCH();
    return DC_OK;
}
