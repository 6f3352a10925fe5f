// Pointwise passes of the ConvLSTM v8 front-end (reference networks/rnn.py:32-79 `ConvLSTMCell_v1`, :371-469 `ConvGRUBlocks_v8`,
// :739-779 `FeatureFusionBlock_v2`, :783-791 `UpscalePS`).  The cell's convolution over cat(x, h) is a fused conv block
// (dc_conv3x3_fwd with two sources, bias, no activation); what remains are
//   the state update   c_next = s(f) * c_cur + s(i) * tanh(g),  h_next = s(o) * tanh(c_next)      cc (B,4C,P) = [i | f | o | g]
//   the hand-over      pre = relu(a + (h_prev + h_new) / 2),    up = PixelShuffle(2)(tanh(pre))
// each one pass per direction, float4 where the plane size allows.  The backwards recompute the gates / the tanh from what
// the forward read or wrote: nothing but cc and c_cur (cell) and pre (hand-over) is kept per frame.  Every thread owns the
// elements it writes: no atomics, two runs give the same bits.  sigmoid and tanh are the accurate expf / tanhf (not __expf):
// the states are carried over the frames of a sequence.
#include "lstm_dev.h"            // lstm_sigmoid, lstm_fwd1, handover_pre, handover_d, LSTM_BLOCK, lstm_grid, all16: shared with lstm_infer.hip, gru_c2f.hip

namespace dc {

struct LstmBwd { float di, df, dO, dg, dc; };
__device__ __forceinline__ LstmBwd lstm_bwd1(float ci, float cf, float co, float cg, float c, float gh, float gc) {
    const float i = lstm_sigmoid(ci), f = lstm_sigmoid(cf), o = lstm_sigmoid(co), g = tanhf(cg);
    const float t = tanhf(f * c + i * g);
    const float dc = gc + gh * o * (1.f - t * t);                       // gradient of c_next
    LstmBwd r;
    r.dO = gh * t * o * (1.f - o);
    r.di = dc * g * i * (1.f - i);
    r.df = dc * c * f * (1.f - f);
    r.dg = dc * i * (1.f - g * g);
    r.dc = dc * f;
    return r;
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

// grid (x, B): blockIdx.y is the batch item; a batch item is CP = C * P floats per tensor (4 CP of cc).  The gate planes sit CP
// floats apart, so the float4 body exists only where CP % 4 == 0 (and the bases are 16-byte aligned); the scalar loop takes
// what the body leaves -- everything otherwise.
__global__ __launch_bounds__(LSTM_BLOCK) void lstm_cell_fwd_kernel(const float* __restrict__ cc, const float* __restrict__ c_cur,
                                                                  float* __restrict__ h_next, float* __restrict__ c_next, unsigned CP) {
    const size_t b = blockIdx.y;
    const float* ci = cc + b * 4 * CP;
    const float* cf = ci + CP;
    const float* co = cf + CP;
    const float* cg = co + CP;
    const float* c0 = c_cur + b * CP;
    float* hn = h_next + b * CP;
    float* cn = c_next + b * CP;
    const bool vec = (CP & 3) == 0 && aligned16(ci) && aligned16(c0) && aligned16(hn) && aligned16(cn);
    const unsigned nv = vec ? CP >> 2 : 0, tid = blockIdx.x * LSTM_BLOCK + threadIdx.x, step = gridDim.x * LSTM_BLOCK;
    for (unsigned j = tid; j < nv; j += step) {
        const float4 vi = reinterpret_cast<const float4*>(ci)[j], vf = reinterpret_cast<const float4*>(cf)[j];
        const float4 vo = reinterpret_cast<const float4*>(co)[j], vg = reinterpret_cast<const float4*>(cg)[j];
        const float4 vc = reinterpret_cast<const float4*>(c0)[j];
        const LstmFwd r0 = lstm_fwd1(vi.x, vf.x, vo.x, vg.x, vc.x), r1 = lstm_fwd1(vi.y, vf.y, vo.y, vg.y, vc.y);
        const LstmFwd r2 = lstm_fwd1(vi.z, vf.z, vo.z, vg.z, vc.z), r3 = lstm_fwd1(vi.w, vf.w, vo.w, vg.w, vc.w);
        reinterpret_cast<float4*>(hn)[j] = make_float4(r0.h, r1.h, r2.h, r3.h);
        reinterpret_cast<float4*>(cn)[j] = make_float4(r0.c, r1.c, r2.c, r3.c);
    }
    for (unsigned j = (nv << 2) + tid; j < CP; j += step) {
        const LstmFwd r = lstm_fwd1(ci[j], cf[j], co[j], cg[j], c0[j]);
        hn[j] = r.h;
        cn[j] = r.c;
    }
}

// g_h / g_c may be NULL (a zero gradient)
__global__ __launch_bounds__(LSTM_BLOCK) void lstm_cell_bwd_kernel(const float* __restrict__ cc, const float* __restrict__ c_cur,
                                                                  const float* __restrict__ g_h, const float* __restrict__ g_c,
                                                                  float* __restrict__ d_cc, float* __restrict__ d_c_cur, unsigned CP) {
    const size_t b = blockIdx.y;
    const float* ci = cc + b * 4 * CP;
    const float* cf = ci + CP;
    const float* co = cf + CP;
    const float* cg = co + CP;
    const float* c0 = c_cur + b * CP;
    const float* gh = g_h ? g_h + b * CP : nullptr;
    const float* gc = g_c ? g_c + b * CP : nullptr;
    float* di = d_cc + b * 4 * CP;
    float* df = di + CP;
    float* dO = df + CP;
    float* dg = dO + CP;
    float* dc = d_c_cur + b * CP;
    const bool vec = (CP & 3) == 0 && aligned16(ci) && aligned16(c0) && aligned16(gh) && aligned16(gc) && aligned16(di) && aligned16(dc);
    const unsigned nv = vec ? CP >> 2 : 0, tid = blockIdx.x * LSTM_BLOCK + threadIdx.x, step = gridDim.x * LSTM_BLOCK;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (unsigned j = tid; j < nv; j += step) {
        const float4 vi = reinterpret_cast<const float4*>(ci)[j], vf = reinterpret_cast<const float4*>(cf)[j];
        const float4 vo = reinterpret_cast<const float4*>(co)[j], vg = reinterpret_cast<const float4*>(cg)[j];
        const float4 vc = reinterpret_cast<const float4*>(c0)[j];
        const float4 a = gh ? reinterpret_cast<const float4*>(gh)[j] : zero, e = gc ? reinterpret_cast<const float4*>(gc)[j] : zero;
        const LstmBwd r0 = lstm_bwd1(vi.x, vf.x, vo.x, vg.x, vc.x, a.x, e.x), r1 = lstm_bwd1(vi.y, vf.y, vo.y, vg.y, vc.y, a.y, e.y);
        const LstmBwd r2 = lstm_bwd1(vi.z, vf.z, vo.z, vg.z, vc.z, a.z, e.z), r3 = lstm_bwd1(vi.w, vf.w, vo.w, vg.w, vc.w, a.w, e.w);
        reinterpret_cast<float4*>(di)[j] = make_float4(r0.di, r1.di, r2.di, r3.di);
        reinterpret_cast<float4*>(df)[j] = make_float4(r0.df, r1.df, r2.df, r3.df);
        reinterpret_cast<float4*>(dO)[j] = make_float4(r0.dO, r1.dO, r2.dO, r3.dO);
        reinterpret_cast<float4*>(dg)[j] = make_float4(r0.dg, r1.dg, r2.dg, r3.dg);
        reinterpret_cast<float4*>(dc)[j] = make_float4(r0.dc, r1.dc, r2.dc, r3.dc);
    }
    for (unsigned j = (nv << 2) + tid; j < CP; j += step) {
        const LstmBwd r = lstm_bwd1(ci[j], cf[j], co[j], cg[j], c0[j], gh ? gh[j] : 0.f, gc ? gc[j] : 0.f);
        di[j] = r.di;
        df[j] = r.df;
        dO[j] = r.dO;
        dg[j] = r.dg;
        dc[j] = r.dc;
    }
}

// ---- coarse-to-fine hand-over ---------------------------------------------------------------------------------------------
// PixelShuffle(2): up[b, q, 2y + i, 2x + j] = tanh(pre[b, 4q + 2i + j, y, x])   (handover_pre: lstm_dev.h)
// d(pre pre-ReLU) from the two consumers of pre: handover_d (lstm_dev.h)

// Vector form (w % 4 == 0, 16-byte aligned bases): a thread takes the four channels 4q..4q+3 at four neighbouring pixels of a
// row: 12 float4 loads, 4 float4 stores of pre and 4 float4 stores of up (two output rows of eight pixels).
// items = B * (C/4) * h * (w/4)
__global__ __launch_bounds__(LSTM_BLOCK) void lstm_handover_fwd_vec_kernel(const float* __restrict__ a, const float* __restrict__ h_prev,
                                                                          const float* __restrict__ h_new, float* __restrict__ pre,
                                                                          float* __restrict__ up, unsigned items, int h, int w) {
    const unsigned w4 = w >> 2, P = (unsigned)h * w;
    for (unsigned it = blockIdx.x * LSTM_BLOCK + threadIdx.x; it < items; it += gridDim.x * LSTM_BLOCK) {
        const unsigned x4 = it % w4, r = it / w4, y = r % h, bq = r / h;          // bq = b * (C/4) + q
        const size_t in0 = (size_t)bq * 4 * P + (size_t)y * w + 4 * x4;
        float4 p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const size_t o = in0 + (size_t)k * P;
            const float4 va = *reinterpret_cast<const float4*>(a + o), vp = *reinterpret_cast<const float4*>(h_prev + o);
            const float4 vn = *reinterpret_cast<const float4*>(h_new + o);
            p[k] = make_float4(handover_pre(va.x, vp.x, vn.x), handover_pre(va.y, vp.y, vn.y), handover_pre(va.z, vp.z, vn.z),
                               handover_pre(va.w, vp.w, vn.w));
            *reinterpret_cast<float4*>(pre + o) = p[k];
        }
        if (up) {
            float* u0 = up + (size_t)bq * 4 * P + (size_t)(2 * y) * (2 * w) + 8 * x4;       // (2h, 2w) plane of 4 P floats
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float4 e = p[2 * i], o = p[2 * i + 1];                                 // j = 0 / 1
                float* row = u0 + (size_t)i * 2 * w;
                *reinterpret_cast<float4*>(row) = make_float4(tanhf(e.x), tanhf(o.x), tanhf(e.y), tanhf(o.y));
                *reinterpret_cast<float4*>(row + 4) = make_float4(tanhf(e.z), tanhf(o.z), tanhf(e.w), tanhf(o.w));
            }
        }
    }
}
// Scalar form: one element of pre per thread; n = B * C * P
__global__ __launch_bounds__(LSTM_BLOCK) void lstm_handover_fwd_kernel(const float* __restrict__ a, const float* __restrict__ h_prev,
                                                                      const float* __restrict__ h_new, float* __restrict__ pre,
                                                                      float* __restrict__ up, unsigned n, int h, int w) {
    const unsigned P = (unsigned)h * w;
    for (unsigned e = blockIdx.x * LSTM_BLOCK + threadIdx.x; e < n; e += gridDim.x * LSTM_BLOCK) {
        const float v = handover_pre(a[e], h_prev[e], h_new[e]);
        pre[e] = v;
        if (up) {
            const unsigned x = e % w, r = e / w, y = r % h, bc = r / h, k = bc & 3, bq = bc >> 2;
            up[(size_t)bq * 4 * P + (size_t)(2 * y + (k >> 1)) * (2 * w) + 2 * x + (k & 1)] = tanhf(v);
        }
    }
}

// g_pre / g_up may be NULL (zero); d_a / d_h_prev / d_h_new may be NULL (not wanted)
__global__ __launch_bounds__(LSTM_BLOCK) void lstm_handover_bwd_vec_kernel(const float* __restrict__ pre, const float* __restrict__ g_pre,
                                                                          const float* __restrict__ g_up, float* __restrict__ d_a,
                                                                          float* __restrict__ d_h_prev, float* __restrict__ d_h_new,
                                                                          unsigned items, int h, int w) {
    const unsigned w4 = w >> 2, P = (unsigned)h * w;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (unsigned it = blockIdx.x * LSTM_BLOCK + threadIdx.x; it < items; it += gridDim.x * LSTM_BLOCK) {
        const unsigned x4 = it % w4, r = it / w4, y = r % h, bq = r / h;
        const size_t in0 = (size_t)bq * 4 * P + (size_t)y * w + 4 * x4;
        float4 gu[4] = {zero, zero, zero, zero};                                              // per channel k, pixels x..x+3
        if (g_up) {
            const float* u0 = g_up + (size_t)bq * 4 * P + (size_t)(2 * y) * (2 * w) + 8 * x4;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float* row = u0 + (size_t)i * 2 * w;
                const float4 lo = *reinterpret_cast<const float4*>(row), hi = *reinterpret_cast<const float4*>(row + 4);
                gu[2 * i] = make_float4(lo.x, lo.z, hi.x, hi.z);
                gu[2 * i + 1] = make_float4(lo.y, lo.w, hi.y, hi.w);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const size_t o = in0 + (size_t)k * P;
            const float4 vp = *reinterpret_cast<const float4*>(pre + o);
            const float4 gp = g_pre ? *reinterpret_cast<const float4*>(g_pre + o) : zero;
            const float4 d = make_float4(handover_d(vp.x, gp.x, gu[k].x), handover_d(vp.y, gp.y, gu[k].y),
                                         handover_d(vp.z, gp.z, gu[k].z), handover_d(vp.w, gp.w, gu[k].w));
            const float4 half = make_float4(d.x * 0.5f, d.y * 0.5f, d.z * 0.5f, d.w * 0.5f);
            if (d_a) *reinterpret_cast<float4*>(d_a + o) = d;
            if (d_h_prev) *reinterpret_cast<float4*>(d_h_prev + o) = half;
            if (d_h_new) *reinterpret_cast<float4*>(d_h_new + o) = half;
        }
    }
}
__global__ __launch_bounds__(LSTM_BLOCK) void lstm_handover_bwd_kernel(const float* __restrict__ pre, const float* __restrict__ g_pre,
                                                                      const float* __restrict__ g_up, float* __restrict__ d_a,
                                                                      float* __restrict__ d_h_prev, float* __restrict__ d_h_new,
                                                                      unsigned n, int h, int w) {
    const unsigned P = (unsigned)h * w;
    for (unsigned e = blockIdx.x * LSTM_BLOCK + threadIdx.x; e < n; e += gridDim.x * LSTM_BLOCK) {
        float gu = 0.f;
        if (g_up) {
            const unsigned x = e % w, r = e / w, y = r % h, bc = r / h, k = bc & 3, bq = bc >> 2;
            gu = g_up[(size_t)bq * 4 * P + (size_t)(2 * y + (k >> 1)) * (2 * w) + 2 * x + (k & 1)];
        }
        const float d = handover_d(pre[e], g_pre ? g_pre[e] : 0.f, gu);
        if (d_a) d_a[e] = d;
        if (d_h_prev) d_h_prev[e] = d * 0.5f;
        if (d_h_new) d_h_new[e] = d * 0.5f;
    }
}

}  // namespace dc

using namespace dc;

// every tensor of a call stays below 2^31 elements (cc is the largest: 4 B C P)
static bool lstm_ok(int B, int C, int P) {
    return B > 0 && B <= 65535 && C > 0 && P > 0 && (size_t)B * 4 * C * P < (1ull << 31);
}

extern "C" int dc_lstm_block(void) { return LSTM_BLOCK; }

extern "C" int dc_lstm_cell_fwd(const float* cc, const float* c_cur, float* h_next, float* c_next, int B, int C, int P, void* stream) {
    if (!cc || !c_cur || !h_next || !c_next || !lstm_ok(B, C, P)) return DC_EINVAL;
    const unsigned CP = (unsigned)C * P;
    const size_t work = (CP & 3) ? CP : CP >> 2;
    hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3(lstm_grid(work), B), dim3(LSTM_BLOCK), 0, (hipStream_t)stream, cc, c_cur, h_next, c_next, CP);
    DC_CHECK_LAUNCH();
    return DC_OK;
}
extern "C" int dc_lstm_cell_bwd(const float* cc, const float* c_cur, const float* g_h, const float* g_c, float* d_cc, float* d_c_cur,
                                int B, int C, int P, void* stream) {
    if (!cc || !c_cur || !d_cc || !d_c_cur || !lstm_ok(B, C, P)) return DC_EINVAL;
    const unsigned CP = (unsigned)C * P;
    const size_t work = (CP & 3) ? CP : CP >> 2;
    hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3(lstm_grid(work), B), dim3(LSTM_BLOCK), 0, (hipStream_t)stream, cc, c_cur, g_h, g_c, d_cc,
                       d_c_cur, CP);
    DC_CHECK_LAUNCH();
    return DC_OK;
}

static bool handover_ok(int B, int C, int h, int w) {
    return B > 0 && C > 0 && (C & 3) == 0 && h > 0 && w > 0 && (size_t)B * C * h * w < (1ull << 31);
}

extern "C" int dc_lstm_handover_fwd(const float* a, const float* h_prev, const float* h_new, float* pre, float* up, int B, int C, int h,
                                    int w, void* stream) {
    if (!a || !h_prev || !h_new || !pre || !handover_ok(B, C, h, w)) return DC_EINVAL;
    const size_t n = (size_t)B * C * h * w;
    if ((w & 3) == 0 && all16({a, h_prev, h_new, pre, up})) {
        const size_t items = n >> 4;
        hipLaunchKernelGGL(lstm_handover_fwd_vec_kernel, dim3(lstm_grid(items)), dim3(LSTM_BLOCK), 0, (hipStream_t)stream, a, h_prev, h_new,
                           pre, up, (unsigned)items, h, w);
    } else {
        hipLaunchKernelGGL(lstm_handover_fwd_kernel, dim3(lstm_grid(n)), dim3(LSTM_BLOCK), 0, (hipStream_t)stream, a, h_prev, h_new, pre, up,
                           (unsigned)n, h, w);
    }
    DC_CHECK_LAUNCH();
    return DC_OK;
}
extern "C" int dc_lstm_handover_bwd(const float* pre, const float* g_pre, const float* g_up, float* d_a, float* d_h_prev, float* d_h_new,
                                    int B, int C, int h, int w, void* stream) {
    if (!pre || (!d_a && !d_h_prev && !d_h_new) || !handover_ok(B, C, h, w)) return DC_EINVAL;
    const size_t n = (size_t)B * C * h * w;
    if ((w & 3) == 0 && all16({pre, g_pre, g_up, d_a, d_h_prev, d_h_new})) {
        const size_t items = n >> 4;
        hipLaunchKernelGGL(lstm_handover_bwd_vec_kernel, dim3(lstm_grid(items)), dim3(LSTM_BLOCK), 0, (hipStream_t)stream, pre, g_pre, g_up,
                           d_a, d_h_prev, d_h_new, (unsigned)items, h, w);
    } else {
        hipLaunchKernelGGL(lstm_handover_bwd_kernel, dim3(lstm_grid(n)), dim3(LSTM_BLOCK), 0, (hipStream_t)stream, pre, g_pre, g_up, d_a,
                           d_h_prev, d_h_new, (unsigned)n, h, w);
    }
    DC_CHECK_LAUNCH();
    return DC_OK;
}
