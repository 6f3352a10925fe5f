// Pointwise passes of the ConvLSTM v8 front-end (reference networks/rnn.py:32-79 `ConvLSTMCell_v1`, :371-469 `ConvGRUBlocks_v8`,
// :739-779 `FeatureFusionBlock_v2`, :783-791 `UpscalePS`).  The cell's convolution over cat(x, h) is a fused conv block
// (dc_conv3x3_fwd with two sources, bias, no activation); what remains are
//   the state update   c_next = s(f) * c_cur + s(i) * tanh(g),  h_next = s(o) * tanh(c_next)      cc (B,4C,P) = [i | f | o | g]
//   the hand-over      pre = relu(a + (h_prev + h_new) / 2),    up = PixelShuffle(2)(tanh(pre))
// each one pass per direction, float4 where the plane size allows.  The backwards recompute the gates / the tanh from what
// the forward read or wrote: nothing but cc and c_cur (cell) and pre (hand-over) is kept per frame.  Every thread owns the
// elements it writes: no atomics, two runs give the same bits.  sigmoid and tanh are the accurate expf / tanhf (not __expf):
// the states are carried over the frames of a sequence.
#include "c2f_dev.h"             // the hand-over walk; through it lstm_dev.h: lstm_sigmoid, lstm_fwd1, LSTM_BLOCK, lstm_grid

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

// ---- coarse-to-fine hand-over: the item walk of c2f_dev.h with the cell "h_new is given" ------------------------------------
struct GivenCell {
    const float *h_prev, *h_new;
    template <class V> struct S { V hp, hn; };
    template <class V> __device__ __forceinline__ S<V> eval(unsigned, size_t o) const { return {ld<V>(h_prev + o), ld<V>(h_new + o)}; }
    template <class V> __device__ __forceinline__ void store(size_t, const S<V>&) const {}
};
// d_a = d, d_h_prev = d_h_new = d / 2, each where wanted
struct GivenCellBwd {
    float *d_a, *d_h_prev, *d_h_new;
    template <class V> __device__ __forceinline__ void bwd(unsigned, size_t o, V pre, V gp, V gu) const {
        const V d = handover_d(pre, gp, gu), half = halve(d);
        if (d_a) st(d_a + o, d);
        if (d_h_prev) st(d_h_prev + o, half);
        if (d_h_new) st(d_h_new + o, half);
    }
};

// VEC: 12 float4 loads, 4 float4 stores of pre and 4 of up per item; up may be NULL
template <bool VEC>
__global__ __launch_bounds__(LSTM_BLOCK) void lstm_handover_fwd_kernel(const float* __restrict__ a, const float* __restrict__ h_prev,
                                                                      const float* __restrict__ h_new, float* __restrict__ pre,
                                                                      float* __restrict__ up, unsigned n, int C, int h, int w) {
    handover_fwd_walk<VEC, false>(GivenCell{h_prev, h_new}, a, nullptr, pre, up, (size_t)C * h * w, n, C, h, w);
}
// g_pre / g_up may be NULL (zero); d_a / d_h_prev / d_h_new may be NULL (not wanted)
template <bool VEC>
__global__ __launch_bounds__(LSTM_BLOCK) void lstm_handover_bwd_kernel(const float* __restrict__ pre, const float* __restrict__ g_pre,
                                                                      const float* __restrict__ g_up, float* __restrict__ d_a,
                                                                      float* __restrict__ d_h_prev, float* __restrict__ d_h_new,
                                                                      unsigned n, int C, int h, int w) {
    handover_bwd_walk<VEC>(GivenCellBwd{d_a, d_h_prev, d_h_new}, pre, g_pre, g_up, n, C, h, w);
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

static bool handover_ok(int B, int C, int h, int w, size_t* n) { return (C & 3) == 0 && c2f_sizes(B, C, h, w, 1, n); }

extern "C" int dc_lstm_handover_fwd(const float* a, const float* h_prev, const float* h_new, float* pre, float* up, int B, int C, int h,
                                    int w, void* stream) {
    size_t n;
    if (!a || !h_prev || !h_new || !pre || !handover_ok(B, C, h, w, &n)) return DC_EINVAL;
    const bool vec = c2f_vec(C, w, up, (size_t)C * h * w, {a, h_prev, h_new, pre, up});
    const C2fLaunch l = c2f_launch(vec, n);
    hipLaunchKernelGGL(vec ? lstm_handover_fwd_kernel<true> : lstm_handover_fwd_kernel<false>, dim3(l.grid), dim3(LSTM_BLOCK), 0,
                       (hipStream_t)stream, a, h_prev, h_new, pre, up, l.count, C, h, w);
    DC_CHECK_LAUNCH();
    return DC_OK;
}
extern "C" int dc_lstm_handover_bwd(const float* pre, const float* g_pre, const float* g_up, float* d_a, float* d_h_prev, float* d_h_new,
                                    int B, int C, int h, int w, void* stream) {
    size_t n;
    if (!pre || (!d_a && !d_h_prev && !d_h_new) || !handover_ok(B, C, h, w, &n)) return DC_EINVAL;
    const bool vec = c2f_vec(C, w, nullptr, 0, {pre, g_pre, g_up, d_a, d_h_prev, d_h_new});
    const C2fLaunch l = c2f_launch(vec, n);
    hipLaunchKernelGGL(vec ? lstm_handover_bwd_kernel<true> : lstm_handover_bwd_kernel<false>, dim3(l.grid), dim3(LSTM_BLOCK), 0,
                       (hipStream_t)stream, pre, g_pre, g_up, d_a, d_h_prev, d_h_new, l.count, C, h, w);
    DC_CHECK_LAUNCH();
    return DC_OK;
}
