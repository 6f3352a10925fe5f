// Inference form of the ConvGRU v5 cell step (reference evaluate_depth_gru_fusion.py:504-554 `evaluate_v5_seq`) for B independent
// streams, ALL feature levels in one launch.  No trace and no backward, so the state is rewritten in place and the residual that
// feeds the decoder leaves the same pass:
//   dc_gru_infer_rh:    rh = r * h                                         r = gates[:, :C]
//   dc_gru_infer_tail:  h_next = (1 - u) * h + u * cnm                     u = gates[:, C:]
//                       out    = f + (h_next + h) / 2 ;   h <- h_next      (6 streams where blend + residual move 8)
//   dc_gru_infer_init:  state[l][b] = h0[l]  for b < B                     (the learned initial state, broadcast over the streams)
// The level descriptors travel by value as kernel arguments (as GatherArgs in gru.hip: no table upload); blockIdx.y is the
// level, x strides over its elements -- the grid is sized for the largest level and the blocks of a small one fall through
// their loop.  float4 where a level's pointers and C*P allow it (every batch row, and the update half of the gates, then start
// on a 16-byte boundary), scalar otherwise: level 4 of a 64 x 96 input has P = 6.
// The arithmetic is left uncontracted: each product and sum rounds once, in the order written, which is what the framework's
// elementwise expression gives -- the reference a test holds these kernels to.
#include "dc_common.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace dc {

constexpr int GRU_INFER_MAX = 8;
struct GruInferArgs {
    dc_gru_infer_level lv[GRU_INFER_MAX];
    int B;
};
struct GruInitArgs {
    const float* h0[GRU_INFER_MAX];
    float* state[GRU_INFER_MAX];
    unsigned M[GRU_INFER_MAX];
    int B;
};

__device__ __forceinline__ bool aligned16(const void* a, const void* b, const void* c) {
    return ((((size_t)a) | ((size_t)b) | ((size_t)c)) & 15) == 0;
}

__global__ __launch_bounds__(256) void gru_infer_rh_kernel(GruInferArgs a) {
    const dc_gru_infer_level& L = a.lv[blockIdx.y];
    const unsigned CP = (unsigned)L.C * (unsigned)L.P, n = (unsigned)a.B * CP;
    const float* __restrict__ gates = L.gates;
    const float* __restrict__ h = L.h;
    float* __restrict__ rh = L.rh;
    const unsigned stride = gridDim.x * 256;
    if ((CP & 3) == 0 && aligned16(gates, h, rh)) {
        const unsigned CP4 = CP >> 2, n4 = n >> 2;
        for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
            const unsigned b = i / CP4, r = i - b * CP4;
            const float4 g = reinterpret_cast<const float4*>(gates)[b * 2 * CP4 + r];
            const float4 hv = reinterpret_cast<const float4*>(h)[i];
            float4 o;
            o.x = g.x * hv.x; o.y = g.y * hv.y; o.z = g.z * hv.z; o.w = g.w * hv.w;
            reinterpret_cast<float4*>(rh)[i] = o;
        }
    } else {
        for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
            const unsigned b = i / CP, r = i - b * CP;
            rh[i] = gates[b * 2 * CP + r] * h[i];
        }
    }
}

// one element: h_next = (1 - u) h + u cnm (rnn.py:141), out = f + (h_next + h) / 2 (evaluate_depth_gru_fusion.py:544)
__device__ __forceinline__ void tail1(float u, float hv, float c, float fv, float& hn, float& o) {
    const float p = (1.f - u) * hv;
    const float q = u * c;
    hn = p + q;
    const float s = hn + hv;
    o = fv + s / 2.f;
}

__global__ __launch_bounds__(256) void gru_infer_tail_kernel(GruInferArgs a) {
    const dc_gru_infer_level& L = a.lv[blockIdx.y];
    const unsigned CP = (unsigned)L.C * (unsigned)L.P, n = (unsigned)a.B * CP;
    const float* __restrict__ gates = L.gates;
    const float* __restrict__ cnm = L.cnm;
    const float* __restrict__ f = L.f;
    float* h = L.h;                                  // read, then rewritten: the same element by the same thread
    float* __restrict__ out = L.out;
    const unsigned stride = gridDim.x * 256;
    if ((CP & 3) == 0 && aligned16(gates, cnm, f) && aligned16(h, out, nullptr)) {
        const unsigned CP4 = CP >> 2, n4 = n >> 2;
        for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
            const unsigned b = i / CP4, r = i - b * CP4;
            const float4 u = reinterpret_cast<const float4*>(gates)[b * 2 * CP4 + CP4 + r];
            const float4 hv = reinterpret_cast<const float4*>(h)[i];
            const float4 c = reinterpret_cast<const float4*>(cnm)[i];
            const float4 fv = reinterpret_cast<const float4*>(f)[i];
            float4 hn, o;
            tail1(u.x, hv.x, c.x, fv.x, hn.x, o.x);
            tail1(u.y, hv.y, c.y, fv.y, hn.y, o.y);
            tail1(u.z, hv.z, c.z, fv.z, hn.z, o.z);
            tail1(u.w, hv.w, c.w, fv.w, hn.w, o.w);
            reinterpret_cast<float4*>(h)[i] = hn;
            reinterpret_cast<float4*>(out)[i] = o;
        }
    } else {
        for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
            const unsigned b = i / CP, r = i - b * CP;
            float hn, o;
            tail1(gates[b * 2 * CP + CP + r], h[i], cnm[i], f[i], hn, o);
            h[i] = hn;
            out[i] = o;
        }
    }
}

__global__ __launch_bounds__(256) void gru_infer_init_kernel(GruInitArgs a) {
    const int l = blockIdx.y;
    const unsigned M = a.M[l], n = (unsigned)a.B * M;
    const float* __restrict__ src = a.h0[l];
    float* __restrict__ dst = a.state[l];
    const unsigned stride = gridDim.x * 256;
    if ((M & 3) == 0 && aligned16(src, dst, nullptr)) {
        const unsigned M4 = M >> 2, n4 = n >> 2;
        for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n4; i += stride)
            reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i % M4];
    } else {
        for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += stride) dst[i] = src[i % M];
    }
}

// blocks in x for the largest level: 256 threads, a float4 each where the level takes that path, 4096 at the most
static unsigned infer_grid(size_t most) { return (unsigned)std::min<size_t>(std::max<size_t>((most + 255) / 256, 1), 4096); }

// fills `a` from the host array; `tail`: which pointers the launch needs.  false: refuse (DC_EINVAL)
static bool infer_args(const dc_gru_infer_level* lv, int nlev, int B, bool tail, GruInferArgs& a, size_t& most) {
    if (!lv || nlev < 1 || nlev > GRU_INFER_MAX || B <= 0) return false;
    most = 0;
    for (int l = 0; l < nlev; ++l) {
        const dc_gru_infer_level& L = lv[l];
        if (!L.gates || !L.h || L.C <= 0 || L.P <= 0) return false;
        if (tail ? (!L.cnm || !L.f || !L.out) : !L.rh) return false;
        const size_t CP = (size_t)L.C * (size_t)L.P;
        if ((size_t)B * 2 * CP >= (1ull << 31)) return false;                  // the gates, the largest tensor: 32-bit indices
        most = std::max(most, (CP & 3) == 0 ? (size_t)B * CP / 4 : (size_t)B * CP);
        a.lv[l] = L;
    }
    a.B = B;
    return true;
}

}  // namespace dc

using namespace dc;

extern "C" int dc_gru_infer_rh(const dc_gru_infer_level* lv, int nlev, int B, void* stream) {
    GruInferArgs a{};
    size_t most;
    if (!infer_args(lv, nlev, B, false, a, most)) return DC_EINVAL;
    hipLaunchKernelGGL(gru_infer_rh_kernel, dim3(infer_grid(most), nlev), dim3(256), 0, (hipStream_t)stream, a);
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" int dc_gru_infer_tail(const dc_gru_infer_level* lv, int nlev, int B, void* stream) {
    GruInferArgs a{};
    size_t most;
    if (!infer_args(lv, nlev, B, true, a, most)) return DC_EINVAL;
    hipLaunchKernelGGL(gru_infer_tail_kernel, dim3(infer_grid(most), nlev), dim3(256), 0, (hipStream_t)stream, a);
    DC_CHECK_LAUNCH();
    return DC_OK;
}

extern "C" int dc_gru_infer_init(const float* const* h0, float* const* state, const size_t* M, int nlev, int B, void* stream) {
    if (!h0 || !state || !M || nlev < 1 || nlev > GRU_INFER_MAX || B <= 0) return DC_EINVAL;
    GruInitArgs a{};
    size_t most = 0;
    for (int l = 0; l < nlev; ++l) {
        if (!h0[l] || !state[l] || M[l] == 0 || (size_t)B * M[l] >= (1ull << 31)) return DC_EINVAL;
        a.h0[l] = h0[l]; a.state[l] = state[l]; a.M[l] = (unsigned)M[l];
        most = std::max(most, (M[l] & 3) == 0 ? (size_t)B * M[l] / 4 : (size_t)B * M[l]);
    }
    a.B = B;
    hipLaunchKernelGGL(gru_infer_init_kernel, dim3(infer_grid(most), nlev), dim3(256), 0, (hipStream_t)stream, a);
    DC_CHECK_LAUNCH();
    return DC_OK;
}
