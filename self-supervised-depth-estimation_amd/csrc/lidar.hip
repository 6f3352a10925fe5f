// Velodyne scans -> sparse depth maps (reference kitti_utils.py:46-98 generate_depth_map, datasets/kitti_dataset.py:71-86
// get_depth, export_gt_depth.py).  include/depthcore.h: dc_lidar_depth_maps.
//
// Three passes over a batch of scans, all on the caller's stream:
//   clear    -- the workspace: key planes and "earliest" side planes to all ones, "latest" side planes to zero;
//   project  -- one thread per point: fp64 projection in numpy's unfused order, then a 32-bit atomicMin of the order-preserving
//               key of the fp32 depth into the pixel; points that land in column 0 or W-1 also record, per row, the earliest
//               point (64-bit atomicMin of the index) and the latest point with its depth (64-bit atomicMax of index << 32 | bits);
//   finalize -- one thread per OUTPUT pixel: gather through the nearest-neighbour tables, apply the reference's edge-column
//               grouping, clamp negatives, mirror, store.
// Integer min / max commute, so the result does not depend on the order in which points arrive: two calls give the same bits.
// This file is built with -ffp-contract=off: numpy does not fuse.
#include <algorithm>

#include "dc_common.h"

namespace {

constexpr uint32_t kEmptyKey = 0xFFFFFFFFu;
constexpr unsigned long long kEmpty64 = ~0ull;

// fp32 -> uint32 whose unsigned order is the float order (negative values included); no finite or infinite value maps to kEmptyKey
__device__ __forceinline__ uint32_t depth_key(float d) {
    const uint32_t b = __builtin_bit_cast(uint32_t, d);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_depth(uint32_t k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// workspace, in 64-bit words: [n_img key planes of key_words each | earliest (n_img, 2, max_h) | latest (n_img, 2, max_h)]
struct LidarWs {
    size_t key_words;      // 64-bit words of one key plane (max_w * max_h keys, rounded up to even)
    size_t ones_words;     // words cleared to all ones: the key planes and `earliest`
    size_t total_words;
    int max_h;
};

LidarWs ws_layout(int n_img, int max_w, int max_h) {
    LidarWs w;
    w.key_words = ((size_t)max_w * max_h + 1) / 2;
    const size_t side = (size_t)n_img * 2 * max_h;
    w.ones_words = (size_t)n_img * w.key_words + side;
    w.total_words = w.ones_words + side;
    w.max_h = max_h;
    return w;
}

__global__ __launch_bounds__(256) void lidar_clear_kernel(unsigned long long* ws, size_t ones_words, size_t total_words) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total_words; i += (size_t)gridDim.x * 256)
        ws[i] = i < ones_words ? kEmpty64 : 0ull;
}

__global__ __launch_bounds__(256) void lidar_project_kernel(const float4* __restrict__ points, const dc_lidar_img* __restrict__ desc,
                                                            unsigned long long* ws, LidarWs L, int n_img) {
    const int img = blockIdx.y;
    const dc_lidar_img& d = desc[img];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.n_points) return;
    const float4 p = points[d.point_off + i];
    if (!(p.x >= 0.f)) return;                                  // kitti_utils.py:67
    const double x = p.x, y = p.y, z = p.z;                     // column 3 is replaced by 1 (:13)
    const double q0 = ((d.P[0] * x + d.P[1] * y) + d.P[2] * z) + d.P[3];
    const double q1 = ((d.P[4] * x + d.P[5] * y) + d.P[6] * z) + d.P[7];
    const double q2 = ((d.P[8] * x + d.P[9] * y) + d.P[10] * z) + d.P[11];
    const double px = rint(q0 / q2) - 1.0, py = rint(q1 / q2) - 1.0;     // :71, :78-79 (np.round: half to even)
    if (!(px >= 0.0 && py >= 0.0 && px < (double)d.W && py < (double)d.H)) return;      // :80-81; NaN fails
    const int ix = (int)px, iy = (int)py;
    const float depth = d.vel_depth ? p.x : (float)q2;          // :73-74
    uint32_t* keys = reinterpret_cast<uint32_t*>(ws + (size_t)img * L.key_words);
    atomicMin(&keys[(size_t)iy * d.W + ix], depth_key(depth));
    if (ix == 0 || ix == d.W - 1) {
        unsigned long long* earliest = ws + (size_t)n_img * L.key_words;
        unsigned long long* latest = earliest + (size_t)n_img * 2 * L.max_h;
        const size_t slot = ((size_t)img * 2 + (ix != 0)) * L.max_h + iy;
        atomicMin(&earliest[slot], (unsigned long long)i);
        atomicMax(&latest[slot], ((unsigned long long)i << 32) | __builtin_bit_cast(uint32_t, depth));
    }
}

__global__ __launch_bounds__(256) void lidar_finalize_kernel(const dc_lidar_img* __restrict__ desc, const unsigned long long* __restrict__ ws,
                                                             LidarWs L, int n_img, const int32_t* __restrict__ rows,
                                                             const int32_t* __restrict__ cols, int Ho, int Wo, float* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n_img * Ho * Wo) return;
    const int xo = (int)(idx % Wo), yo = (int)((idx / Wo) % Ho), img = (int)(idx / ((size_t)Wo * Ho));
    const dc_lidar_img& d = desc[img];
    const int W = d.W, H = d.H;
    const int ny = rows[(size_t)img * Ho + yo];
    const int nx = cols[(size_t)img * Wo + (d.flip ? Wo - 1 - xo : xo)];      // fliplr follows the resize
    const uint32_t* keys = reinterpret_cast<const uint32_t*>(ws + (size_t)img * L.key_words);
    uint32_t key = keys[(size_t)ny * W + nx];
    float v = 0.f;
    if (key != kEmptyKey) {
        bool latest_wins = false;
        if (nx == 0 || nx == W - 1) {
            // sub2ind (:39-43, :89) gives (y, W-1) and (y+1, 0) one key: when both are hit, the pixel of the group's earliest
            // point takes the minimum over both (:91-95), the other keeps its last-written depth (:86)
            const int side = nx != 0, py = side ? ny + 1 : ny - 1;
            if (py >= 0 && py < H) {
                const unsigned long long* earliest = ws + (size_t)n_img * L.key_words;
                const unsigned long long* latest = earliest + (size_t)n_img * 2 * L.max_h;
                const unsigned long long e_other = earliest[((size_t)img * 2 + (1 - side)) * L.max_h + py];
                if (e_other != kEmpty64) {
                    const size_t me = ((size_t)img * 2 + side) * L.max_h + ny;
                    if (earliest[me] < e_other) {
                        key = min(key, keys[(size_t)py * W + (side ? 0 : W - 1)]);
                    } else {
                        latest_wins = true;
                        v = __builtin_bit_cast(float, (uint32_t)latest[me]);
                    }
                }
            }
        }
        if (!latest_wins) v = key_depth(key);
        v = v < 0.f ? 0.f : v;                                  // :96
    }
    out[idx] = v;
}

}  // namespace

extern "C" size_t dc_lidar_workspace_bytes(int n_img, int max_w, int max_h) {
    if (n_img <= 0 || n_img > 65535 || max_w < 2 || max_w > 65535 || max_h <= 0 || max_h > 65535 || (size_t)max_w * max_h > (1u << 28)) return 0;
    return ws_layout(n_img, max_w, max_h).total_words * sizeof(unsigned long long);
}

extern "C" int dc_lidar_depth_maps(const float* points, size_t n_points, const dc_lidar_img* desc_host, const dc_lidar_img* desc_dev,
                                   int n_img, const int32_t* rows_host, const int32_t* rows_dev, const int32_t* cols_host,
                                   const int32_t* cols_dev, int Ho, int Wo, float* out, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    if (!points || ((size_t)points & 15) || !desc_host || !desc_dev || !rows_host || !rows_dev || !cols_host || !cols_dev || !out ||
        !workspace || ((size_t)workspace & 7) || n_img <= 0 || n_img > 65535 || Ho <= 0 || Ho > 65535 || Wo <= 0 || Wo > 65535 ||
        (size_t)Ho * Wo > (1u << 28))
        return DC_EINVAL;
    int max_w = 0, max_h = 0, max_n = 0;
    for (int i = 0; i < n_img; ++i) {
        const dc_lidar_img& d = desc_host[i];
        if (d.W < 2 || d.W > 65535 || d.H <= 0 || d.H > 65535 || (size_t)d.W * d.H > (1u << 28)) return DC_EINVAL;
        if (d.n_points < 0 || d.point_off < 0 || (size_t)d.point_off > n_points || (size_t)d.n_points > n_points - (size_t)d.point_off)
            return DC_EINVAL;
        for (int y = 0; y < Ho; ++y)
            if (rows_host[(size_t)i * Ho + y] < 0 || rows_host[(size_t)i * Ho + y] >= d.H) return DC_EINVAL;
        for (int x = 0; x < Wo; ++x)
            if (cols_host[(size_t)i * Wo + x] < 0 || cols_host[(size_t)i * Wo + x] >= d.W) return DC_EINVAL;
        max_w = std::max(max_w, d.W);
        max_h = std::max(max_h, d.H);
        max_n = std::max(max_n, d.n_points);
    }
    const LidarWs L = ws_layout(n_img, max_w, max_h);
    if (workspace_bytes < L.total_words * sizeof(unsigned long long)) return DC_EWORKSPACE;
    const size_t out_blocks = ((size_t)n_img * Ho * Wo + 255) / 256;
    if (out_blocks > 0x7FFFFFFFull) return DC_EINVAL;
    unsigned long long* ws = (unsigned long long*)workspace;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lidar_clear_kernel, dim3((unsigned)std::min<size_t>((L.total_words + 255) / 256, 4096)), dim3(256), 0, st, ws,
                       L.ones_words, L.total_words);
    if (max_n > 0)
        hipLaunchKernelGGL(lidar_project_kernel, dim3((max_n + 255) / 256, n_img), dim3(256), 0, st, (const float4*)points, desc_dev, ws, L,
                           n_img);
    hipLaunchKernelGGL(lidar_finalize_kernel, dim3((unsigned)out_blocks), dim3(256), 0, st, desc_dev, (const unsigned long long*)ws, L,
                       n_img, rows_dev, cols_dev, Ho, Wo, out);
    DC_CHECK_LAUNCH();
    return DC_OK;
}
