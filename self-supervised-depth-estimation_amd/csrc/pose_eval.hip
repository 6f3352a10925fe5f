// Trajectory scoring of the pose evaluation: the reference's evaluate_pose.py:23-46 (dump_xyz, compute_ate) and :104-125 (the
// ground-truth local poses, the snippets, np.mean / np.std).  include/depthcore.h: dc_pose_ate.
//
// A KITTI odometry sequence has 1,101-4,541 frames and a snippet is a chain of at most track_length - 1 4x4 products: this is
// not where the evaluation's time goes.  One thread per snippet, everything in fp64 as numpy's, nothing tuned -- the point is
// that the predictions never leave the device and that the host receives ates | mean | std with one copy.
//   pa_ate_kernel     snippet i: the chains over pred[i : i+L-1] and over the ground-truth local poses, walked twice (sums for
//                     the scale, then the error) instead of being stored
//   pa_stats_kernel   one block: mean and population std in two passes (as np.std), thread t taking entries t, t + 256, ... in
//                     order and a fixed tree -- two calls give the same bits
// Built with -ffp-contract=off (Makefile): plain IEEE multiplies and adds, as numpy's.
#include "dc_common.h"

namespace dc {

constexpr int PA_THREADS = 256;

struct Aff {                    // [A | t] over the implicit row (0,0,0,1)
    double a[3][3], t[3];
};

__device__ __forceinline__ Aff pa_load(const double* g) {          // one (3,4) row-major row of poses/XX.txt
    Aff m;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) m.a[r][c] = g[4 * r + c];
        m.t[r] = g[4 * r + 3];
    }
    return m;
}

__device__ __forceinline__ Aff pa_mul(const Aff& x, const Aff& y) {
    Aff m;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) m.a[r][c] = (x.a[r][0] * y.a[0][c] + x.a[r][1] * y.a[1][c]) + x.a[r][2] * y.a[2][c];
        m.t[r] = ((x.a[r][0] * y.t[0] + x.a[r][1] * y.t[1]) + x.a[r][2] * y.t[2]) + x.t[r];
    }
    return m;
}

// the GENERAL affine inverse [A^-1 | -A^-1 t] by the adjugate -- not [A^T | -A^T t]: the pose files carry six decimals, so
// their rotation blocks are orthogonal to ~1e-6 only and np.linalg.inv does not assume they are
__device__ __forceinline__ Aff pa_inv(const Aff& x) {
    const double (&a)[3][3] = x.a;
    const double c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1];
    const double c01 = a[1][2] * a[2][0] - a[1][0] * a[2][2];
    const double c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0];
    const double det = (a[0][0] * c00 + a[0][1] * c01) + a[0][2] * c02;
    Aff m;
    m.a[0][0] = c00 / det;
    m.a[0][1] = (a[0][2] * a[2][1] - a[0][1] * a[2][2]) / det;
    m.a[0][2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) / det;
    m.a[1][0] = c01 / det;
    m.a[1][1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) / det;
    m.a[1][2] = (a[0][2] * a[1][0] - a[0][0] * a[1][2]) / det;
    m.a[2][0] = c02 / det;
    m.a[2][1] = (a[0][1] * a[2][0] - a[0][0] * a[2][1]) / det;
    m.a[2][2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) / det;
#pragma unroll
    for (int r = 0; r < 3; ++r) m.t[r] = -((m.a[r][0] * x.t[0] + m.a[r][1] * x.t[1]) + m.a[r][2] * x.t[2]);
    return m;
}

// evaluate_pose.py:111-114: ground-truth local pose j = inv(inv(G[j]) G[j+1])
__device__ __forceinline__ Aff pa_gt_local(const double* gt, int j) {
    return pa_inv(pa_mul(pa_inv(pa_load(gt + (size_t)12 * j)), pa_load(gt + (size_t)12 * (j + 1))));
}

// dump_xyz (evaluate_pose.py:23-30) of both trajectories of snippet i, one point pair at a time: point 0 is the origin, point
// k the translation column of C_k = C_{k-1} T[i+k-1].  The predictions are full 4x4 matrices (their last row is multiplied
// through as np.dot does), widened from fp32 on load.
template <class F>
__device__ __forceinline__ void pa_walk(const float* pred, const double* gt, int i, int npts, F&& point) {
    double C[4][4] = {{1., 0., 0., 0.}, {0., 1., 0., 0.}, {0., 0., 1., 0.}, {0., 0., 0., 1.}};
    Aff G;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) G.a[r][c] = r == c ? 1. : 0.;
        G.t[r] = 0.;
    }
    const double zero[3] = {0., 0., 0.};
    point(zero, zero);
    for (int k = 1; k < npts; ++k) {
        const float* T = pred + (size_t)16 * (i + k - 1);
        double n[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                n[r][c] = ((C[r][0] * (double)T[c] + C[r][1] * (double)T[4 + c]) + C[r][2] * (double)T[8 + c]) + C[r][3] * (double)T[12 + c];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) C[r][c] = n[r][c];
        G = pa_mul(G, pa_gt_local(gt, i + k - 1));
        const double p[3] = {C[0][3], C[1][3], C[2][3]};
        point(G.t, p);
    }
}

// compute_ate (evaluate_pose.py:34-46) of snippet i = blockIdx.x * 256 + threadIdx.x < S
__global__ __launch_bounds__(PA_THREADS) void pa_ate_kernel(const float* __restrict__ pred, const double* __restrict__ gt,
                                                            double* __restrict__ ates, int S, int track_length) {
    const int i = blockIdx.x * PA_THREADS + threadIdx.x;
    if (i >= S) return;
    // pred[i : i+L-1] and gt_local[i : i+L-1] both hold S entries: the slices are clipped at S, the last snippets are shorter
    const int npts = 1 + min(track_length - 1, S - i);
    double off[3] = {0., 0., 0.}, sgp = 0., spp = 0.;
    int k = 0;
    pa_walk(pred, gt, i, npts, [&](const double* g, const double* p) {
        if (k++ == 0) {
#pragma unroll
            for (int d = 0; d < 3; ++d) off[d] = g[d] - p[d];                       // the first points coincide
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double q = p[d] + off[d];
            sgp += g[d] * q;
            spp += q * q;
        }
    });
    const double scale = sgp / spp;                       // 0 / 0 = NaN when all predicted points coincide, as numpy's
    double see = 0.;
    pa_walk(pred, gt, i, npts, [&](const double* g, const double* p) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double e = (p[d] + off[d]) * scale - g[d];
            see += e * e;
        }
    });
    ates[i] = sqrt(see) / (double)npts;
}

__device__ __forceinline__ double pa_block_sum(double v, double* sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// out[S] = np.mean(ates), out[S + 1] = np.std(ates) (population, two passes)
__global__ __launch_bounds__(PA_THREADS) void pa_stats_kernel(double* __restrict__ out, int S) {
    __shared__ double sm[PA_THREADS / 64];
    double acc = 0.;
    for (int i = threadIdx.x; i < S; i += PA_THREADS) acc += out[i];
    const double mean = pa_block_sum(acc, sm) / (double)S;
    acc = 0.;
    for (int i = threadIdx.x; i < S; i += PA_THREADS) {
        const double d = out[i] - mean;
        acc += d * d;
    }
    const double var = pa_block_sum(acc, sm) / (double)S;
    if (threadIdx.x == 0) {
        out[S] = mean;
        out[S + 1] = sqrt(var);
    }
}

}  // namespace dc

using namespace dc;

extern "C" int dc_pose_ate(const float* pred, const double* gt_global, double* out, int N, int M, int track_length, void* stream) {
    if (!pred || !gt_global || !out || M < 2 || N != M - 1 || track_length < 1) return DC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int S = M - 1;
    hipLaunchKernelGGL(pa_ate_kernel, dim3(ceil_div(S, PA_THREADS)), dim3(PA_THREADS), 0, st, pred, gt_global, out, S, track_length);
    DC_CHECK_LAUNCH();
    hipLaunchKernelGGL(pa_stats_kernel, dim3(1), dim3(PA_THREADS), 0, st, out, S);
    DC_CHECK_LAUNCH();
    return DC_OK;
}
