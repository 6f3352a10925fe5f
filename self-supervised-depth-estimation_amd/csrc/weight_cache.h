// The per-step prepared-weight cache (weight_cache.hip: dc_wino_cache_*): the look-ups the three kernel families that keep
// prepared weights in it launch through, and the Winograd weight transform that wino.hip's per-launch kernel and the cache's batched
// refresh share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace dc {

constexpr int PSK = 8;                // reduction channels per staged chunk of wino_ps_kernel: the chunking of U's staging order

#ifdef __HIPCC__
// U = G g G^T for every (m, k), written in staging order.  grid over padded (Mp x Kp); one thread per (m, k).
template <bool DGRAD>
__device__ __forceinline__ void wino_weight_one(const float* __restrict__ w, float* __restrict__ uhat, int idx, int Co, int Ci, int MT,
                                                int Mp, int Kp, int WK) {
    // 256 consecutive threads = a 16 (m) x 16 (k) tile with m fastest: the 16-byte stores of 16 consecutive m are one
    // 256-byte run (the staging order has m innermost), and the filter reads stay efficient -- 16 consecutive k of a row are
    // 576 contiguous bytes (forward), 16 consecutive m are (data gradient).  With k fastest the batched launch spent 310 us
    // on 440 MB: every store instruction scattered 16-byte pieces 256 bytes apart.
    const int tiles_k = (Kp + 15) >> 4;
    const int tile = idx >> 8, within = idx & 255;
    const int m = (tile / tiles_k) * 16 + (within & 15), k = (tile % tiles_k) * 16 + (within >> 4);
    if (m >= Mp || k >= Kp) return;
    const int M = DGRAD ? Ci : Co, K = DGRAD ? Co : Ci;
    float g[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float v = 0.f;
            if (m < M && k < K)
                v = DGRAD ? w[((size_t)k * Ci + m) * 9 + (2 - i) * 3 + (2 - j)] : w[((size_t)m * Ci + k) * 9 + i * 3 + j];
            g[i][j] = v;
        }
    float t[4][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        t[0][j] = g[0][j];
        t[1][j] = 0.5f * (g[0][j] + g[1][j] + g[2][j]);
        t[2][j] = 0.5f * (g[0][j] - g[1][j] + g[2][j]);
        t[3][j] = g[2][j];
    }
    float u[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        u[i][0] = t[i][0];
        u[i][1] = 0.5f * (t[i][0] + t[i][1] + t[i][2]);
        u[i][2] = 0.5f * (t[i][0] - t[i][1] + t[i][2]);
        u[i][3] = t[i][2];
    }
    const int mb = m / MT, mi = m - mb * MT, kc = k / WK, kin = k - kc * WK;
    const int nchunks = Kp / WK;
    float* dst = uhat + ((((size_t)mb * nchunks + kc) * WK + kin) * 4) * MT * 4 + (size_t)mi * 4;
#pragma unroll
    for (int pq = 0; pq < 4; ++pq)
        *reinterpret_cast<float4*>(dst + (size_t)pq * MT * 4) = make_float4(u[pq][0], u[pq][1], u[pq][2], u[pq][3]);
}
#endif
static inline int wino_wblocks(int Mp, int Kp) { return (Mp / 16) * ((Kp + 15) / 16); }   // 16 x 16 tiles of wino_weight_one

// The prepared weights of a REGISTERED weight that is fresh after a refresh, or nullptr: then the caller prepares them into its
// workspace as before (an unseen variant gets its buffer here and joins the next refresh; nothing is allocated while `st` is
// being captured).
//   Winograd U of (weight, pass, MT): (Mp, Kp) = the padded (rows, reduction channels)
const float* wc_lookup(const float* w, int Ci, int Co, bool dgrad, int MT, int Mp, int Kp, hipStream_t st);
//   the bf16 direct kernels' prepared weights of (weight, pass, MT) (conv_bf16.hip)
const void* wc_lookup_c3b(const float* w, int Ci, int Co, int dgrad, int MT, int nmblk, int nchunks, hipStream_t st);
//   the split 1x1 weights of (weight, direction) (gemm1x1_x3.hip)
const void* wc_lookup_x3(const float* w, int Ci, int Co, int tr, int Mp, int K, hipStream_t st);

}  // namespace dc
