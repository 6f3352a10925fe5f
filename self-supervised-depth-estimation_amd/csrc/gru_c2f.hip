// Joins of the coarse-to-fine ConvGRU front-end, gru_version v10 (reference networks/rnn.py:472-569 `ConvGRUBlocks_v9` with
// attention=False, :101-143 `ConvGRUCell`, :739-779 `FeatureFusionBlock_v2`, :783-791 `UpscalePS`; trainer_gru.py:716-764
// `run_gru_v9_v10`, evaluate_depth_gru_fusion_my_v.py:641-701 `evaluate_v9_v10_seq`).  The cell's two convolutions are fused
// conv blocks and r * h is dc_gru_rh / dc_gru_infer_rh; what is left of a frame at one scale is the GRU's tail and the block's
// hand-over, ONE launch here where v5's and v8's parts would take two (dc_gru_blend_* and dc_lstm_handover_*):
//   h_new = (1 - u) * h_prev + u * cnm          u = gates[:, C:2C]   (gates (B, 2C, h, w) = [reset | update], post-sigmoid)
//   pre   = relu(a + (h_prev + h_new) / 2)      a = resConfUnit1(input_1)
//   up    = PixelShuffle(2)(tanh(pre))          up[b, q, 2y + i, 2x + j] = tanh(pre[b, 4q + 2i + j, y, x])
// The item walk is lstm.hip's hand-over (four channels 4q..4q+3 at four neighbouring pixels per thread where C % 4 == 0,
// w % 4 == 0 and the bases are 16-byte aligned; one element per thread otherwise) and the per-element expressions are those of
// gru.hip's blend and lstm_dev.h's hand-over, in their order.  The backward recomputes u and the tanh from what the forward read
// or wrote: per frame only gates, h_prev, cnm and pre are kept.  Every thread owns what it writes: no atomics, two runs give the
// same bits; no allocation or synchronisation: capturable.  tanh is the accurate tanhf: the state is carried over the frames.
#include "lstm_dev.h"            // handover_pre, handover_d, LSTM_BLOCK, lstm_grid, all16

namespace dc {

__device__ __forceinline__ float gru_blend1(float u, float h, float cnm) { return (1.f - u) * h + u * cnm; }      // rnn.py:136

__device__ __forceinline__ float4 gru_blend4(float4 u, float4 h, float4 c) {
    return make_float4(gru_blend1(u.x, h.x, c.x), gru_blend1(u.y, h.y, c.y), gru_blend1(u.z, h.z, c.z), gru_blend1(u.w, h.w, c.w));
}
__device__ __forceinline__ float4 handover_pre4(float4 a, float4 hp, float4 hn) {
    return make_float4(handover_pre(a.x, hp.x, hn.x), handover_pre(a.y, hp.y, hn.y), handover_pre(a.z, hp.z, hn.z),
                       handover_pre(a.w, hp.w, hn.w));
}
// the item's 16 values of tanh(p) as two output rows of eight pixels; u0: element (2y, 2 * 4 x4) of the item's (2h, 2w) plane
__device__ __forceinline__ void shuffle_store(float* u0, const float4 (&p)[4], int w) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float4 e = p[2 * i], o = p[2 * i + 1];                             // j = 0 / 1
        float* row = u0 + (size_t)i * 2 * w;
        *reinterpret_cast<float4*>(row) = make_float4(tanhf(e.x), tanhf(o.x), tanhf(e.y), tanhf(o.y));
        *reinterpret_cast<float4*>(row + 4) = make_float4(tanhf(e.z), tanhf(o.z), tanhf(e.w), tanhf(o.w));
    }
}

// Where an item or an element lives.  b: batch item, q: channel quad, (yy, 4 x4): first pixel;  items = B * (C/4) * h * (w/4)
struct C2fItem { unsigned b, q, yy, x4; };
__device__ __forceinline__ C2fItem c2f_item(unsigned it, unsigned w4, int h, unsigned C4) {
    C2fItem r;
    r.x4 = it % w4;
    const unsigned t = it / w4, bq = t / h;
    r.yy = t % h;
    r.q = bq % C4;
    r.b = bq / C4;
    return r;
}
// shuffled position of element (channel ch, pixel (yy, x)) inside a batch item's (C/4, 2h, 2w) block
__device__ __forceinline__ size_t shuffled(unsigned rem, unsigned P, int h, int w) {
    const unsigned x = rem % w, t = rem / w, yy = t % h, ch = t / h, k = ch & 3, q = ch >> 2;
    return (size_t)q * 4 * P + (size_t)(2 * yy + (k >> 1)) * (2 * w) + 2 * x + (k & 1);
}

// ---- training forward ------------------------------------------------------------------------------------------------------
// Vector form: per channel four float4 loads (u, h_prev, cnm, a) and two float4 stores (h_new, pre); up as shuffle_store.
__global__ __launch_bounds__(LSTM_BLOCK) void gru_handover_fwd_vec_kernel(const float* __restrict__ gates, const float* __restrict__ h_prev,
                                                                         const float* __restrict__ cnm, const float* __restrict__ a,
                                                                         float* __restrict__ h_new, float* __restrict__ pre,
                                                                         float* __restrict__ up, unsigned items, int C, int h, int w) {
    const unsigned w4 = w >> 2, P = (unsigned)h * w, C4 = C >> 2;
    const size_t CP = (size_t)C * P;
    for (unsigned it = blockIdx.x * LSTM_BLOCK + threadIdx.x; it < items; it += gridDim.x * LSTM_BLOCK) {
        const C2fItem m = c2f_item(it, w4, h, C4);
        const size_t in0 = (size_t)m.b * CP + (size_t)m.q * 4 * P + (size_t)m.yy * w + 4 * m.x4;
        const float* u0 = gates + (size_t)m.b * CP + CP + in0;                   // update gate of channel 4q: b * 2CP + CP + ...
        float4 p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const size_t o = in0 + (size_t)k * P;
            const float4 vu = *reinterpret_cast<const float4*>(u0 + (size_t)k * P), vh = *reinterpret_cast<const float4*>(h_prev + o);
            const float4 vc = *reinterpret_cast<const float4*>(cnm + o), va = *reinterpret_cast<const float4*>(a + o);
            const float4 hn = gru_blend4(vu, vh, vc);
            p[k] = handover_pre4(va, vh, hn);
            *reinterpret_cast<float4*>(h_new + o) = hn;
            *reinterpret_cast<float4*>(pre + o) = p[k];
        }
        if (up) shuffle_store(up + (size_t)m.b * CP + (size_t)m.q * 4 * P + (size_t)(2 * m.yy) * (2 * w) + 8 * m.x4, p, w);
    }
}
// Scalar form: one element per thread; n = B * C * P
__global__ __launch_bounds__(LSTM_BLOCK) void gru_handover_fwd_kernel(const float* __restrict__ gates, const float* __restrict__ h_prev,
                                                                     const float* __restrict__ cnm, const float* __restrict__ a,
                                                                     float* __restrict__ h_new, float* __restrict__ pre,
                                                                     float* __restrict__ up, unsigned n, int C, int h, int w) {
    const unsigned P = (unsigned)h * w, CP = (unsigned)C * P;
    for (unsigned e = blockIdx.x * LSTM_BLOCK + threadIdx.x; e < n; e += gridDim.x * LSTM_BLOCK) {
        const unsigned b = e / CP, rem = e - b * CP;
        const float hp = h_prev[e];
        const float hn = gru_blend1(gates[(size_t)b * 2 * CP + CP + rem], hp, cnm[e]);
        const float v = handover_pre(a[e], hp, hn);
        h_new[e] = hn;
        pre[e] = v;
        if (up) up[(size_t)b * CP + shuffled(rem, P, h, w)] = tanhf(v);
    }
}

// ---- training backward -----------------------------------------------------------------------------------------------------
//   d = (pre > 0) * (g_pre + unshuffle(g_up) * (1 - tanh(pre)^2));   G = g_h_new + d / 2
//   d_a = d;  d_cnm = G * u;  d_gates = [0 | G * (cnm - h_prev)];  d_h_prev = d / 2 + G * (1 - u)
struct C2fBwd { float da, dcnm, du, dh; };
__device__ __forceinline__ C2fBwd gru_handover_bwd1(float u, float hp, float cn, float pre, float gh, float gp, float gu) {
    C2fBwd r;
    r.da = handover_d(pre, gp, gu);
    const float half = r.da * 0.5f, G = gh + half;
    r.dcnm = G * u;
    r.du = G * (cn - hp);
    r.dh = half + G * (1.f - u);
    return r;
}
// g_h_new / g_pre / g_up may be NULL (zero)
__global__ __launch_bounds__(LSTM_BLOCK) void gru_handover_bwd_vec_kernel(const float* __restrict__ gates, const float* __restrict__ h_prev,
                                                                         const float* __restrict__ cnm, const float* __restrict__ pre,
                                                                         const float* __restrict__ g_h_new, const float* __restrict__ g_pre,
                                                                         const float* __restrict__ g_up, float* __restrict__ d_gates,
                                                                         float* __restrict__ d_h_prev, float* __restrict__ d_cnm,
                                                                         float* __restrict__ d_a, unsigned items, int C, int h, int w) {
    const unsigned w4 = w >> 2, P = (unsigned)h * w, C4 = C >> 2;
    const size_t CP = (size_t)C * P;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (unsigned it = blockIdx.x * LSTM_BLOCK + threadIdx.x; it < items; it += gridDim.x * LSTM_BLOCK) {
        const C2fItem m = c2f_item(it, w4, h, C4);
        const size_t in0 = (size_t)m.b * CP + (size_t)m.q * 4 * P + (size_t)m.yy * w + 4 * m.x4;
        const size_t r0 = (size_t)m.b * CP + in0;                                 // reset half of the gates, channel 4q; update: + CP
        float4 gu[4] = {zero, zero, zero, zero};                                  // per channel k, pixels x..x+3
        if (g_up) {
            const float* s0 = g_up + (size_t)m.b * CP + (size_t)m.q * 4 * P + (size_t)(2 * m.yy) * (2 * w) + 8 * m.x4;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float* row = s0 + (size_t)i * 2 * w;
                const float4 lo = *reinterpret_cast<const float4*>(row), hi = *reinterpret_cast<const float4*>(row + 4);
                gu[2 * i] = make_float4(lo.x, lo.z, hi.x, hi.z);
                gu[2 * i + 1] = make_float4(lo.y, lo.w, hi.y, hi.w);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const size_t o = in0 + (size_t)k * P, go = r0 + (size_t)k * P;
            const float4 vu = *reinterpret_cast<const float4*>(gates + go + CP), vh = *reinterpret_cast<const float4*>(h_prev + o);
            const float4 vc = *reinterpret_cast<const float4*>(cnm + o), vp = *reinterpret_cast<const float4*>(pre + o);
            const float4 gh = g_h_new ? *reinterpret_cast<const float4*>(g_h_new + o) : zero;
            const float4 gp = g_pre ? *reinterpret_cast<const float4*>(g_pre + o) : zero;
            const C2fBwd b0 = gru_handover_bwd1(vu.x, vh.x, vc.x, vp.x, gh.x, gp.x, gu[k].x);
            const C2fBwd b1 = gru_handover_bwd1(vu.y, vh.y, vc.y, vp.y, gh.y, gp.y, gu[k].y);
            const C2fBwd b2 = gru_handover_bwd1(vu.z, vh.z, vc.z, vp.z, gh.z, gp.z, gu[k].z);
            const C2fBwd b3 = gru_handover_bwd1(vu.w, vh.w, vc.w, vp.w, gh.w, gp.w, gu[k].w);
            *reinterpret_cast<float4*>(d_a + o) = make_float4(b0.da, b1.da, b2.da, b3.da);
            *reinterpret_cast<float4*>(d_cnm + o) = make_float4(b0.dcnm, b1.dcnm, b2.dcnm, b3.dcnm);
            *reinterpret_cast<float4*>(d_h_prev + o) = make_float4(b0.dh, b1.dh, b2.dh, b3.dh);
            *reinterpret_cast<float4*>(d_gates + go) = zero;
            *reinterpret_cast<float4*>(d_gates + go + CP) = make_float4(b0.du, b1.du, b2.du, b3.du);
        }
    }
}
__global__ __launch_bounds__(LSTM_BLOCK) void gru_handover_bwd_kernel(const float* __restrict__ gates, const float* __restrict__ h_prev,
                                                                     const float* __restrict__ cnm, const float* __restrict__ pre,
                                                                     const float* __restrict__ g_h_new, const float* __restrict__ g_pre,
                                                                     const float* __restrict__ g_up, float* __restrict__ d_gates,
                                                                     float* __restrict__ d_h_prev, float* __restrict__ d_cnm,
                                                                     float* __restrict__ d_a, unsigned n, int C, int h, int w) {
    const unsigned P = (unsigned)h * w, CP = (unsigned)C * P;
    for (unsigned e = blockIdx.x * LSTM_BLOCK + threadIdx.x; e < n; e += gridDim.x * LSTM_BLOCK) {
        const unsigned b = e / CP, rem = e - b * CP;
        const size_t go = (size_t)b * 2 * CP + rem;
        const float gu = g_up ? g_up[(size_t)b * CP + shuffled(rem, P, h, w)] : 0.f;
        const C2fBwd r = gru_handover_bwd1(gates[go + CP], h_prev[e], cnm[e], pre[e], g_h_new ? g_h_new[e] : 0.f, g_pre ? g_pre[e] : 0.f, gu);
        d_a[e] = r.da;
        d_cnm[e] = r.dcnm;
        d_h_prev[e] = r.dh;
        d_gates[go] = 0.f;
        d_gates[go + CP] = r.du;
    }
}

// ---- inference step: B lockstep windows, the state rewritten in place --------------------------------------------------------
// h is read and written through the same pointer (each element by the thread that read it), so it is not __restrict__.
__global__ __launch_bounds__(LSTM_BLOCK) void gru_c2f_infer_step_vec_kernel(const float* __restrict__ gates, const float* __restrict__ cnm,
                                                                           const float* __restrict__ y, const float* __restrict__ r,
                                                                           float* h, float* pre, float* up, size_t up_bstride,
                                                                           unsigned items, int C, int hh, int w) {
    const unsigned w4 = w >> 2, P = (unsigned)hh * w, C4 = C >> 2;
    const size_t CP = (size_t)C * P;
    for (unsigned it = blockIdx.x * LSTM_BLOCK + threadIdx.x; it < items; it += gridDim.x * LSTM_BLOCK) {
        const C2fItem m = c2f_item(it, w4, hh, C4);
        const size_t in0 = (size_t)m.b * CP + (size_t)m.q * 4 * P + (size_t)m.yy * w + 4 * m.x4;
        const float* u0 = gates + (size_t)m.b * CP + CP + in0;
        float4 p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const size_t o = in0 + (size_t)k * P;
            const float4 vu = *reinterpret_cast<const float4*>(u0 + (size_t)k * P), vh = *reinterpret_cast<const float4*>(h + o);
            const float4 vc = *reinterpret_cast<const float4*>(cnm + o);
            const float4 hn = gru_blend4(vu, vh, vc);
            if (y) {
                const float4 vy = *reinterpret_cast<const float4*>(y + o), vr = *reinterpret_cast<const float4*>(r + o);
                p[k] = handover_pre4(make_float4(vy.x + vr.x, vy.y + vr.y, vy.z + vr.z, vy.w + vr.w), vh, hn);
                if (pre) *reinterpret_cast<float4*>(pre + o) = p[k];
            }
            *reinterpret_cast<float4*>(h + o) = hn;
        }
        if (up)                                                                  // (given only with y)
            shuffle_store(up + (size_t)m.b * up_bstride + (size_t)m.q * 4 * P + (size_t)(2 * m.yy) * (2 * w) + 8 * m.x4, p, w);
    }
}
__global__ __launch_bounds__(LSTM_BLOCK) void gru_c2f_infer_step_kernel(const float* __restrict__ gates, const float* __restrict__ cnm,
                                                                       const float* __restrict__ y, const float* __restrict__ r, float* h,
                                                                       float* pre, float* up, size_t up_bstride, unsigned n, int C, int hh,
                                                                       int w) {
    const unsigned P = (unsigned)hh * w, CP = (unsigned)C * P;
    for (unsigned e = blockIdx.x * LSTM_BLOCK + threadIdx.x; e < n; e += gridDim.x * LSTM_BLOCK) {
        const unsigned b = e / CP, rem = e - b * CP;
        const float h_cur = h[e];
        const float hn = gru_blend1(gates[(size_t)b * 2 * CP + CP + rem], h_cur, cnm[e]);
        if (y) {
            const float v = handover_pre(y[e] + r[e], h_cur, hn);
            if (pre) pre[e] = v;
            if (up) up[(size_t)b * up_bstride + shuffled(rem, P, hh, w)] = tanhf(v);
        }
        h[e] = hn;
    }
}

}  // namespace dc

using namespace dc;

// sizes > 0 and every tensor of a call below 2^31 elements (gates is the largest: 2 B C h w); n: B C h w
static bool c2f_ok(int B, int C, int h, int w, size_t* n) {
    if (B <= 0 || C <= 0 || h <= 0 || w <= 0) return false;
    *n = (size_t)B * C * h * w;
    return *n * 2 < (1ull << 31);
}

extern "C" int dc_gru_handover_fwd(const float* gates, const float* h_prev, const float* cnm, const float* a, float* h_new, float* pre,
                                   float* up, int B, int C, int h, int w, void* stream) {
    size_t n;
    if (!gates || !h_prev || !cnm || !a || !h_new || !pre || !c2f_ok(B, C, h, w, &n)) return DC_EINVAL;
    if (up && (C & 3)) return DC_EINVAL;
    if ((C & 3) == 0 && (w & 3) == 0 && all16({gates, h_prev, cnm, a, h_new, pre, up})) {
        const size_t items = n >> 4;
        hipLaunchKernelGGL(gru_handover_fwd_vec_kernel, dim3(lstm_grid(items)), dim3(LSTM_BLOCK), 0, (hipStream_t)stream, gates, h_prev, cnm,
                           a, h_new, pre, up, (unsigned)items, C, h, w);
    } else {
        hipLaunchKernelGGL(gru_handover_fwd_kernel, dim3(lstm_grid(n)), dim3(LSTM_BLOCK), 0, (hipStream_t)stream, gates, h_prev, cnm, a, h_new,
                           pre, up, (unsigned)n, C, h, w);
    }
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" int dc_gru_handover_bwd(const float* gates, const float* h_prev, const float* cnm, const float* pre, const float* g_h_new,
                                   const float* g_pre, const float* g_up, float* d_gates, float* d_h_prev, float* d_cnm, float* d_a, int B,
                                   int C, int h, int w, void* stream) {
    size_t n;
    if (!gates || !h_prev || !cnm || !pre || !d_gates || !d_h_prev || !d_cnm || !d_a || !c2f_ok(B, C, h, w, &n)) return DC_EINVAL;
    if ((!g_h_new && !g_pre && !g_up) || (g_up && (C & 3))) return DC_EINVAL;
    if ((C & 3) == 0 && (w & 3) == 0 && all16({gates, h_prev, cnm, pre, g_h_new, g_pre, g_up, d_gates, d_h_prev, d_cnm, d_a})) {
        const size_t items = n >> 4;
        hipLaunchKernelGGL(gru_handover_bwd_vec_kernel, dim3(lstm_grid(items)), dim3(LSTM_BLOCK), 0, (hipStream_t)stream, gates, h_prev, cnm,
                           pre, g_h_new, g_pre, g_up, d_gates, d_h_prev, d_cnm, d_a, (unsigned)items, C, h, w);
    } else {
        hipLaunchKernelGGL(gru_handover_bwd_kernel, dim3(lstm_grid(n)), dim3(LSTM_BLOCK), 0, (hipStream_t)stream, gates, h_prev, cnm, pre,
                           g_h_new, g_pre, g_up, d_gates, d_h_prev, d_cnm, d_a, (unsigned)n, C, h, w);
    }
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" int dc_gru_c2f_infer_step(const float* gates, const float* cnm, const float* y, const float* r, float* h, float* pre, float* up,
                                     size_t up_bstride, int B, int C, int hh, int w, void* stream) {
    size_t n;
    if (!gates || !cnm || !h || !c2f_ok(B, C, hh, w, &n)) return DC_EINVAL;
    if ((y == nullptr) != (r == nullptr) || ((pre || up) && !y)) return DC_EINVAL;
    if (up && ((C & 3) || up_bstride < (size_t)C * hh * w)) return DC_EINVAL;
    if ((C & 3) == 0 && (w & 3) == 0 && (!up || (up_bstride & 3) == 0) && all16({gates, cnm, y, r, h, pre, up})) {
        const size_t items = n >> 4;
        hipLaunchKernelGGL(gru_c2f_infer_step_vec_kernel, dim3(lstm_grid(items)), dim3(LSTM_BLOCK), 0, (hipStream_t)stream, gates, cnm, y, r, h,
                           pre, up, up_bstride, (unsigned)items, C, hh, w);
    } else {
        hipLaunchKernelGGL(gru_c2f_infer_step_kernel, dim3(lstm_grid(n)), dim3(LSTM_BLOCK), 0, (hipStream_t)stream, gates, cnm, y, r, h, pre,
                           up, up_bstride, (unsigned)n, C, hh, w);
    }
    DC_CHECK_LAUNCH();
    return DC_OK;
}
