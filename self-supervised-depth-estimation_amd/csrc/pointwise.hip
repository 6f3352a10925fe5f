// 1x1 convolutions of the ResNet trunks (stride 1 or 2, no bias: the `downsample` branches and the Bottleneck
// conv1 / conv3, reference networks/resnet_encoder.py:74-98 via torchvision) as fp32-MFMA GEMMs straight on the NCHW
// tensors.  The library runs these small problems (0.2-0.4 GMAC) through NHWC implicit-GEMM kernels wrapped in
// NCHW<->NHWC transposes and zero-fills that cost more than the GEMM; here the stride-2 gather, the scatter of the data
// gradient (with its zeros) and the split reduction of the weight gradient are part of the kernels.
//   forward        y[b,m,p]          = sum_k w[m,k] * x[b,k,s*py,s*px]
//   data gradient  dx[b,k,s*py,s*px] = sum_m w[m,k] * gy[b,m,p]      (0 at the positions the stride skips)
//   weight grad    dw[m,k]           = sum_{b,p} gy[b,m,p] * x[b,k,s*py,s*px]   split over blocks, fixed-order reduce (slab_reduce16_kernel)
// v_mfma_f32_16x16x4_f32, block = 4 waves = 64 outputs x 64 columns, reduction staged through LDS in chunks of 16.
//
// These are the GENERAL kernels (any shape, scalar staging), and below them the routing of every 1x1 convolution.  Three kernel
// families: the split-operand bf16 GEMMs of gemm1x1_x3.hip (the default, dc_set_gemm_split) and the fp32-MFMA tiled GEMMs of
// gemm1x1.hip -- shapes whose pixel count and channel count allow 16-byte staging: every Bottleneck / downsample / pose-decoder
// convolution at the BASELINE sizes -- and these kernels for the rest.  pw_family() picks one per pass; dc_pointwise_* (queries and
// launches: what depthcore/ops.py and depthcore/bnfold.py call) all go through it.  dc_conv1x1_* stay pinned to fp32-MFMA / general
// and dc_gemm1x1x3_* to the split kernels, for A/B comparisons.
#include "dc_common.h"
#include "gemm1x1.h"
#include "gemm1x1_x3.h"
#include "gemm_tiles.h"

#include <algorithm>

namespace dc {

using pf4 = __attribute__((ext_vector_type(4))) float;

constexpr int PT = 64;                 // block tile (both GEMM output dimensions)
constexpr int PK = 16;                 // reduction chunk
constexpr int PLS = PT + 4;            // LDS row stride (floats)

struct PwArgs {
    const float* a;    // forward: w (M x K);  dgrad: w (red x out = M x K);  wgrad: gy
    const float* b;    // forward: x;          dgrad: gy;                      wgrad: x
    float* out;
    int B, M, K;       // conv channels: M = Co, K = Ci
    int Hi, Wi, Ho, Wo, s;
    int splits;        // wgrad
    const float* bias; // forward epilogue: y = act(y + bias[m])   (null: none)
    int act;
};

// ---- shared MFMA core: acc[nt] += A(16 rows of this wave x PK) * B(PK x 64 columns)
// LDS images: At[PK][PLS] (reduction-major, output row fastest), Bt[PK][PLS] (reduction-major, column fastest)
__device__ __forceinline__ void pw_mma(const float (*At)[PLS], const float (*Bt)[PLS], int wave, int lane, pf4 acc[4]) {
#pragma unroll
    for (int ks = 0; ks < PK / 4; ++ks) {
        const float av = At[ks * 4 + (lane >> 4)][wave * 16 + (lane & 15)];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const float bv = Bt[ks * 4 + (lane >> 4)][nt * 16 + (lane & 15)];
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[nt], 0, 0, 0);
        }
    }
}

// forward: grid (ceil(P/64), ceil(M/64), B);  rows = output channels m, columns = output pixels p, reduction = k
__global__ __launch_bounds__(256) void pw_fwd_kernel(PwArgs a) {
    __shared__ float At[PK][PLS], Bt[PK][PLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = blockIdx.x * PT, m0 = blockIdx.y * PT, b = blockIdx.z;
    const int P = a.Ho * a.Wo;
    pf4 acc[4] = {pf4{0, 0, 0, 0}, pf4{0, 0, 0, 0}, pf4{0, 0, 0, 0}, pf4{0, 0, 0, 0}};
    // staging roles
    const int am = tid >> 2, akq = tid & 3;                 // A: w[m0+am][k0 + 4 akq .. +3]
    const int bk = tid >> 4, bpq = tid & 15;                // B: x[k0+bk][pixels p0 + 4 bpq .. +3]
    size_t boff[4]; bool bok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = p0 + 4 * bpq + j;
        bok[j] = p < P;
        const int py = bok[j] ? p / a.Wo : 0, px = bok[j] ? p - py * a.Wo : 0;
        boff[j] = (size_t)(py * a.s) * a.Wi + (size_t)px * a.s;
    }
    const size_t plane = (size_t)a.Hi * a.Wi;
    for (int k0 = 0; k0 < a.K; k0 += PK) {
        float av[4] = {0.f, 0.f, 0.f, 0.f}, bv[4] = {0.f, 0.f, 0.f, 0.f};
        if (m0 + am < a.M) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (k0 + 4 * akq + j < a.K) av[j] = a.a[(size_t)(m0 + am) * a.K + k0 + 4 * akq + j];
        }
        if (k0 + bk < a.K) {
            const float* src = a.b + ((size_t)b * a.K + k0 + bk) * plane;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (bok[j]) bv[j] = src[boff[j]];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            At[4 * akq + j][am] = av[j];
            Bt[bk][4 * bpq + j] = bv[j];
        }
        __syncthreads();
        pw_mma(At, Bt, wave, lane, acc);
    }
    // D layout: row = (lane>>4)*4 + r, column = lane&15
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wave * 16 + (lane >> 4) * 4 + r, p = p0 + nt * 16 + (lane & 15);
            if (m < a.M && p < P)
                a.out[((size_t)b * a.M + m) * P + p] = act_fwd(acc[nt][r] + (a.bias ? a.bias[m] : 0.f), a.act);
        }
}

// data gradient: grid (ceil(P/64), ceil(K/64), B);  rows = input channels k, columns = pixels p of gy, reduction = m.
// Writes every element of dx: the value at (s*py, s*px), zeros at the positions the stride skips (Hi, Wi multiples of s).
__global__ __launch_bounds__(256) void pw_dgrad_kernel(PwArgs a) {
    __shared__ float At[PK][PLS], Bt[PK][PLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = blockIdx.x * PT, c0 = blockIdx.y * PT, b = blockIdx.z;
    const int P = a.Ho * a.Wo;
    pf4 acc[4] = {pf4{0, 0, 0, 0}, pf4{0, 0, 0, 0}, pf4{0, 0, 0, 0}, pf4{0, 0, 0, 0}};
    const int ar = tid >> 4, aoq = tid & 15;                // A: w[m0+ar][c0 + 4 aoq .. +3]  (reduction m, output k)
    const int br = tid >> 4, bpq = tid & 15;                // B: gy[m0+br][p0 + 4 bpq .. +3]
    for (int r0 = 0; r0 < a.M; r0 += PK) {
        float av[4] = {0.f, 0.f, 0.f, 0.f}, bv[4] = {0.f, 0.f, 0.f, 0.f};
        if (r0 + ar < a.M) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (c0 + 4 * aoq + j < a.K) av[j] = a.a[(size_t)(r0 + ar) * a.K + c0 + 4 * aoq + j];
                if (p0 + 4 * bpq + j < P) bv[j] = a.b[((size_t)b * a.M + r0 + br) * P + p0 + 4 * bpq + j];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            At[ar][4 * aoq + j] = av[j];
            Bt[br][4 * bpq + j] = bv[j];
        }
        __syncthreads();
        pw_mma(At, Bt, wave, lane, acc);
    }
    const size_t plane = (size_t)a.Hi * a.Wi;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = c0 + wave * 16 + (lane >> 4) * 4 + r, p = p0 + nt * 16 + (lane & 15);
            if (c >= a.K || p >= P) continue;
            const int py = p / a.Wo, px = p - py * a.Wo;
            float* dst = a.out + ((size_t)b * a.K + c) * plane + (size_t)(py * a.s) * a.Wi + (size_t)px * a.s;
            if (a.s == 1) {
                dst[0] = acc[nt][r];
            } else {                                            // s == 2: the 2x2 cell of this output pixel
                dst[0] = acc[nt][r]; dst[1] = 0.f;
                dst[a.Wi] = 0.f; dst[a.Wi + 1] = 0.f;
            }
        }
}

// weight gradient: grid (splits, ceil(M/64), ceil(K/64));  rows = m, columns = k, reduction = (b, p) in chunks of 16
// pixels of one image; block `split` takes chunks split, split + splits, ... and writes its partial to slab[split][M][K].
__global__ __launch_bounds__(256) void pw_wgrad_kernel(PwArgs a) {
    __shared__ float At[PK][PLS], Bt[PK][PLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * PT, c0 = blockIdx.z * PT;
    const int P = a.Ho * a.Wo;
    const int cpi = (P + PK - 1) / PK, nchunks = a.B * cpi;      // chunks per image / total
    pf4 acc[4] = {pf4{0, 0, 0, 0}, pf4{0, 0, 0, 0}, pf4{0, 0, 0, 0}, pf4{0, 0, 0, 0}};
    const int rr = tid >> 2, pq = tid & 3;                  // A: gy[m0+rr][pc + 4 pq .. +3];  B: x[c0+rr][same pixels]
    const size_t plane = (size_t)a.Hi * a.Wi;
    for (int ch = blockIdx.x; ch < nchunks; ch += a.splits) {
        const int b = ch / cpi, pc = (ch - b * cpi) * PK;
        float av[4] = {0.f, 0.f, 0.f, 0.f}, bv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = pc + 4 * pq + j;
            if (p < P) {
                if (m0 + rr < a.M) av[j] = a.a[((size_t)b * a.M + m0 + rr) * P + p];
                if (c0 + rr < a.K) {
                    const int py = p / a.Wo, px = p - py * a.Wo;
                    bv[j] = a.b[((size_t)b * a.K + c0 + rr) * plane + (size_t)(py * a.s) * a.Wi + (size_t)px * a.s];
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            At[4 * pq + j][rr] = av[j];
            Bt[4 * pq + j][rr] = bv[j];
        }
        __syncthreads();
        pw_mma(At, Bt, wave, lane, acc);
    }
    float* slab = a.out + (size_t)blockIdx.x * a.M * a.K;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wave * 16 + (lane >> 4) * 4 + r, c = c0 + nt * 16 + (lane & 15);
            if (m < a.M && c < a.K) slab[(size_t)m * a.K + c] = acc[nt][r];
        }
}

static int pw_splits(int B, int Ho, int Wo, int M, int K) {
    const int nchunks = B * ceil_div(Ho * Wo, PK);
    const int outer = ceil_div(M, PT) * ceil_div(K, PT);
    return std::max(1, std::min({nchunks / 4 + 1, ceil_div(1024, outer), 256}));
}

__global__ __launch_bounds__(256) void add_inplace_kernel(float* __restrict__ y, const float* __restrict__ a, size_t n) {
    const size_t n4 = n / 4;
    for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256ull) {
        float4 v = reinterpret_cast<float4*>(y)[i];
        const float4 t = reinterpret_cast<const float4*>(a)[i];
        v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
        reinterpret_cast<float4*>(y)[i] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) y[n4 * 4 + threadIdx.x] += a[n4 * 4 + threadIdx.x];
}
int add_inplace(float* y, const float* a, size_t n, hipStream_t st) {
    if ((((size_t)y | (size_t)a) & 15) != 0) return DC_EINVAL;
    hipLaunchKernelGGL(add_inplace_kernel, dim3((unsigned)std::min<size_t>((n / 4 + 255) / 256 + 1, 4096)), dim3(256), 0, st, y, a, n);
    DC_CHECK_LAUNCH();
    return DC_OK;
}

}  // namespace dc

using namespace dc;

static bool pw_shape_ok(int B, int Ci, int Co, int Hi, int Wi, int s) {
    return B > 0 && Ci > 0 && Co > 0 && Hi > 0 && Wi > 0 && (s == 1 || (s == 2 && !(Hi & 1) && !(Wi & 1)));
}

// ---- launches of the general kernels (any shape that passes pw_shape_ok) ---------------------------------------------------------
static PwArgs pw_args(const float* a_, const float* b_, float* out, int B, int Ci, int Co, int Hi, int Wi, int stride) {
    PwArgs a{};
    a.a = a_; a.b = b_; a.out = out; a.B = B; a.M = Co; a.K = Ci; a.Hi = Hi; a.Wi = Wi; a.Ho = Hi / stride; a.Wo = Wi / stride; a.s = stride;
    return a;
}
static int pw_fwd(const float* x, const float* weight, const float* bias, float* y, int B, int Ci, int Co, int Hi, int Wi, int stride,
                  int act, hipStream_t st) {
    if (!x || !weight || !y || act < 0 || act > ACT_LAST) return DC_EINVAL;
    PwArgs a = pw_args(weight, x, y, B, Ci, Co, Hi, Wi, stride);
    a.bias = bias; a.act = act;
    hipLaunchKernelGGL(pw_fwd_kernel, dim3(ceil_div(a.Ho * a.Wo, PT), ceil_div(Co, PT), B), dim3(256), 0, st, a);
    DC_CHECK_LAUNCH();
    return DC_OK;
}
// the addends (nullable) take a pass each: these kernels' scatter epilogue cannot add
static int pw_dgrad(const float* gy, const float* weight, float* dx, const float* addend, const float* addend2, int B, int Ci, int Co,
                    int Hi, int Wi, int stride, hipStream_t st) {
    if (!gy || !weight || !dx) return DC_EINVAL;
    const PwArgs a = pw_args(weight, gy, dx, B, Ci, Co, Hi, Wi, stride);
    hipLaunchKernelGGL(pw_dgrad_kernel, dim3(ceil_div(a.Ho * a.Wo, PT), ceil_div(Ci, PT), B), dim3(256), 0, st, a);
    DC_CHECK_LAUNCH();
    const size_t n = (size_t)B * Ci * Hi * Wi;
    int rc = addend ? add_inplace(dx, addend, n, st) : DC_OK;
    if (rc == DC_OK && addend2) rc = add_inplace(dx, addend2, n, st);
    return rc;
}
static size_t pw_wgrad_workspace(int B, int Ci, int Co, int Hi, int Wi, int stride) {
    return (size_t)pw_splits(B, Hi / stride, Wi / stride, Co, Ci) * Co * Ci * sizeof(float);
}
static int pw_wgrad(const float* x, const float* gy, float* dweight, void* ws, int B, int Ci, int Co, int Hi, int Wi, int stride,
                    hipStream_t st) {
    if (!x || !gy || !dweight || !ws) return DC_EINVAL;
    PwArgs a = pw_args(gy, x, (float*)ws, B, Ci, Co, Hi, Wi, stride);
    a.splits = pw_splits(B, a.Ho, a.Wo, Co, Ci);
    hipLaunchKernelGGL(pw_wgrad_kernel, dim3(a.splits, ceil_div(Co, PT), ceil_div(Ci, PT)), dim3(256), 0, st, a);
    DC_CHECK_LAUNCH();
    hipLaunchKernelGGL(slab_reduce16_kernel<float>, dim3(ceil_div(Co * Ci, 16)), dim3(256), 0, st, (const float*)ws, dweight, a.splits, Co * Ci);
    DC_CHECK_LAUNCH();
    return DC_OK;
}

// =====================================================================================================================
// The dispatcher: which kernel family takes a pass.  Every dc_pointwise_* entry -- the workspace and partial-count queries and
// the three launches -- asks THIS function, so a query and its launch cannot disagree (the partial layouts of the BatchNorm
// epilogues follow each family's own tiles: a count taken for the wrong family is an out-of-bounds epilogue write).  The split
// mode (dc_get_gemm_split) is read on every call.
// =====================================================================================================================
enum PwFamily { FAM_NONE, FAM_X3, FAM_G1, FAM_PW };      // no family takes it (DC_EINVAL) / split bf16 / fp32-MFMA tiled / general

static bool bn_active(const dc_bn_fold* bn) { return bn && (bn->in_scale || bn->stat_part || bn->bwd_part); }

static PwFamily pw_family(int pass, const dc_bn_fold* bn, int B, int Ci, int Co, int Hi, int Wi, int s) {
    if (!pw_shape_ok(B, Ci, Co, Hi, Wi, s)) return FAM_NONE;
    const bool split = dc_get_gemm_split() != 0;
    bool x3, g1, need_g1;      // the split kernels take it / the fp32-MFMA kernels can / nothing else can (the fold has no general kernel)
    switch (pass) {
    case DC_PASS_FWD:
        // With a fold struct the split family is gated on its statistics layout for bn->groups EVEN WHEN no statistics (or nothing at
        // all: every pointer null) are asked for: that is how the folded path has always chosen, and gating on dc_gemm1x1x3_fwd_ok
        // instead would move the shapes whose group boundary falls inside a wave column to the other family.
        x3 = bn ? dc_gemm1x1x3_stat_parts(B, Ci, Co, Hi, Wi, s, bn->groups, nullptr) > 0 : dc_gemm1x1x3_fwd_ok(B, Ci, Co, Hi, Wi, s) != 0;
        g1 = dc_gemm1x1_fwd_ok(B, Ci, Co, Hi, Wi, s);
        need_g1 = bn_active(bn);
        break;
    case DC_PASS_DGRAD:
        need_g1 = bn && bn->bwd_part;      // the BatchNorm-backward epilogue: stride 1, the family the partials were counted for
        x3 = need_g1 ? s == 1 && dc_gemm1x1x3_bwd_parts(B, Ci, Co, Hi, Wi, bn->groups, nullptr) > 0 : dc_gemm1x1x3_dgrad_ok(B, Ci, Co, Hi, Wi, s) != 0;
        g1 = dc_gemm1x1_dgrad_ok(B, Ci, Co, Hi, Wi, s) && !(need_g1 && s != 1);
        break;
    case DC_PASS_WGRAD:
        x3 = dc_gemm1x1x3_wgrad_ok(B, Ci, Co, Hi, Wi, s);
        g1 = dc_gemm1x1_wgrad_ok(B, Ci, Co, Hi, Wi, s);
        need_g1 = bn && bn->in_scale;
        break;
    default:
        return FAM_NONE;
    }
    if (split && x3) return FAM_X3;
    if (g1) return FAM_G1;
    return need_g1 ? FAM_NONE : FAM_PW;
}

// a fold that asks for the partials of one epilogue, for the queries (the pointer is only tested, never followed)
static dc_bn_fold pw_probe_fold(int groups, bool stat, bool bwd) {
    static float mark;
    dc_bn_fold f{};
    f.groups = groups;
    if (stat) f.stat_part = &mark;
    if (bwd) f.bwd_part = &mark;
    return f;
}

extern "C" size_t dc_pointwise_workspace(int pass, const dc_bn_fold* bn, int B, int Ci, int Co, int Hi, int Wi, int stride) {
    size_t n = 0;
    const bool wgrad = pass == DC_PASS_WGRAD;
    switch (pw_family(pass, bn, B, Ci, Co, Hi, Wi, stride)) {
    case FAM_X3: n = wgrad ? dc_gemm1x1x3_wgrad_workspace(B, Ci, Co, Hi, Wi, stride) : dc_gemm1x1x3_workspace(Ci, Co); break;
    case FAM_G1: n = wgrad ? dc_gemm1x1_wgrad_workspace(B, Ci, Co, Hi, Wi, stride) : 0; break;
    case FAM_PW: n = wgrad ? pw_wgrad_workspace(B, Ci, Co, Hi, Wi, stride) : 0; break;
    case FAM_NONE: break;
    }
    return std::max<size_t>(n, 16);
}
extern "C" int dc_pointwise_stat_parts(int B, int Ci, int Co, int Hi, int Wi, int stride, int groups, int* ppg) {
    const dc_bn_fold f = pw_probe_fold(groups, true, false);
    switch (pw_family(DC_PASS_FWD, &f, B, Ci, Co, Hi, Wi, stride)) {
    case FAM_X3: return dc_gemm1x1x3_stat_parts(B, Ci, Co, Hi, Wi, stride, groups, ppg);
    case FAM_G1: return dc_gemm1x1_stat_parts(B, Ci, Co, Hi, Wi, stride, groups, ppg);
    default: return 0;
    }
}
extern "C" int dc_pointwise_bwd_parts(int B, int Ci, int Co, int Hi, int Wi, int stride, int groups, int* ppg) {
    const dc_bn_fold f = pw_probe_fold(groups, false, true);
    switch (pw_family(DC_PASS_DGRAD, &f, B, Ci, Co, Hi, Wi, stride)) {
    case FAM_X3: return dc_gemm1x1x3_bwd_parts(B, Ci, Co, Hi, Wi, groups, ppg);
    case FAM_G1: return dc_gemm1x1_bwd_parts(B, Ci, Co, Hi, Wi, stride, groups, ppg);
    default: return 0;
    }
}
extern "C" int dc_pointwise_fwd(const float* x, const float* weight, const float* bias, float* y, void* ws, int B, int Ci, int Co, int Hi,
                                int Wi, int stride, int act, const dc_bn_fold* bn, void* stream) {
    switch (pw_family(DC_PASS_FWD, bn, B, Ci, Co, Hi, Wi, stride)) {
    case FAM_X3: return g1x3_fwd(x, weight, bias, y, ws, B, Ci, Co, Hi, Wi, stride, act, bn, stream);
    case FAM_G1: return dc_gemm1x1_fwd(x, weight, bias, y, B, Ci, Co, Hi, Wi, stride, act, bn_active(bn) ? bn : nullptr, stream);
    case FAM_PW: return pw_fwd(x, weight, bias, y, B, Ci, Co, Hi, Wi, stride, act, (hipStream_t)stream);
    default: return DC_EINVAL;
    }
}
extern "C" int dc_pointwise_dgrad(const float* gy, const float* weight, float* dx, void* ws, const float* addend, const float* addend2,
                                  int B, int Ci, int Co, int Hi, int Wi, int stride, const dc_bn_fold* bn, void* stream) {
    if (!(bn && bn->bwd_part)) bn = nullptr;      // only the BatchNorm-backward epilogue concerns this pass
    switch (pw_family(DC_PASS_DGRAD, bn, B, Ci, Co, Hi, Wi, stride)) {
    case FAM_X3: return g1x3_dgrad(gy, weight, dx, ws, addend, addend2, B, Ci, Co, Hi, Wi, stride, bn, stream);
    case FAM_G1: return dc_gemm1x1_dgrad(gy, weight, dx, addend, addend2, B, Ci, Co, Hi, Wi, stride, bn, stream);
    case FAM_PW: return pw_dgrad(gy, weight, dx, addend, addend2, B, Ci, Co, Hi, Wi, stride, (hipStream_t)stream);
    default: return DC_EINVAL;
    }
}
extern "C" int dc_pointwise_wgrad(const float* x, const float* gy, float* dweight, void* ws, int B, int Ci, int Co, int Hi, int Wi,
                                  int stride, const dc_bn_fold* bn, void* stream) {
    switch (pw_family(DC_PASS_WGRAD, bn, B, Ci, Co, Hi, Wi, stride)) {
    case FAM_X3: return g1x3_wgrad(x, gy, dweight, ws, B, Ci, Co, Hi, Wi, stride, bn, stream);
    case FAM_G1: return dc_gemm1x1_wgrad(x, gy, dweight, ws, B, Ci, Co, Hi, Wi, stride, bn && bn->in_scale ? bn : nullptr, stream);
    case FAM_PW: return pw_wgrad(x, gy, dweight, ws, B, Ci, Co, Hi, Wi, stride, (hipStream_t)stream);
    default: return DC_EINVAL;
    }
}

// ---- the family-pinned entries (A/B comparisons in tests/ and tools/): fp32-MFMA where the shape allows, else general; never split ----
extern "C" size_t dc_conv1x1_wgrad_workspace(int B, int Ci, int Co, int Hi, int Wi, int stride) {
    if (!pw_shape_ok(B, Ci, Co, Hi, Wi, stride)) return 0;
    if (dc_gemm1x1_wgrad_ok(B, Ci, Co, Hi, Wi, stride)) return dc_gemm1x1_wgrad_workspace(B, Ci, Co, Hi, Wi, stride);
    return pw_wgrad_workspace(B, Ci, Co, Hi, Wi, stride);
}
extern "C" int dc_conv1x1_bias_act_fwd(const float* x, const float* weight, const float* bias, float* y, int B, int Ci, int Co, int Hi,
                                       int Wi, int stride, int act, void* stream) {
    if (!pw_shape_ok(B, Ci, Co, Hi, Wi, stride)) return DC_EINVAL;
    if (dc_gemm1x1_fwd_ok(B, Ci, Co, Hi, Wi, stride))
        return dc_gemm1x1_fwd(x, weight, bias, y, B, Ci, Co, Hi, Wi, stride, act, nullptr, stream);
    return pw_fwd(x, weight, bias, y, B, Ci, Co, Hi, Wi, stride, act, (hipStream_t)stream);
}
extern "C" int dc_conv1x1_fwd(const float* x, const float* weight, float* y, int B, int Ci, int Co, int Hi, int Wi, int stride,
                              void* stream) {
    return dc_conv1x1_bias_act_fwd(x, weight, nullptr, y, B, Ci, Co, Hi, Wi, stride, ACT_NONE, stream);
}
// dx = data gradient + addend + addend2 (both nullable): an input with up to three consumers; the tiled GEMM sums them in its store
// epilogue (every element of dx is written once, densely, at either stride)
extern "C" int dc_conv1x1_dgrad_add2(const float* gy, const float* weight, float* dx, const float* addend, const float* addend2, int B,
                                     int Ci, int Co, int Hi, int Wi, int stride, void* stream) {
    if (!pw_shape_ok(B, Ci, Co, Hi, Wi, stride)) return DC_EINVAL;
    if (dc_gemm1x1_dgrad_ok(B, Ci, Co, Hi, Wi, stride))
        return dc_gemm1x1_dgrad(gy, weight, dx, addend, addend2, B, Ci, Co, Hi, Wi, stride, nullptr, stream);
    return pw_dgrad(gy, weight, dx, addend, addend2, B, Ci, Co, Hi, Wi, stride, (hipStream_t)stream);
}
extern "C" int dc_conv1x1_dgrad_add(const float* gy, const float* weight, float* dx, const float* addend, int B, int Ci, int Co, int Hi,
                                    int Wi, int stride, void* stream) {
    return dc_conv1x1_dgrad_add2(gy, weight, dx, addend, nullptr, B, Ci, Co, Hi, Wi, stride, stream);
}
extern "C" int dc_conv1x1_dgrad(const float* gy, const float* weight, float* dx, int B, int Ci, int Co, int Hi, int Wi, int stride,
                                void* stream) {
    return dc_conv1x1_dgrad_add2(gy, weight, dx, nullptr, nullptr, B, Ci, Co, Hi, Wi, stride, stream);
}
extern "C" int dc_conv1x1_wgrad(const float* x, const float* gy, float* dweight, void* ws, int B, int Ci, int Co, int Hi, int Wi,
                                int stride, void* stream) {
    if (!pw_shape_ok(B, Ci, Co, Hi, Wi, stride)) return DC_EINVAL;
    if (dc_gemm1x1_wgrad_ok(B, Ci, Co, Hi, Wi, stride))
        return dc_gemm1x1_wgrad(x, gy, dweight, ws, B, Ci, Co, Hi, Wi, stride, nullptr, stream);
    return pw_wgrad(x, gy, dweight, ws, B, Ci, Co, Hi, Wi, stride, (hipStream_t)stream);
}

// ... with a BatchNorm folded in (dc_bn_fold): the fp32-MFMA kernels only
extern "C" int dc_conv1x1_bn_ok(int B, int Ci, int Co, int Hi, int Wi) {
    return dc_gemm1x1_fwd_ok(B, Ci, Co, Hi, Wi, 1) && dc_gemm1x1_dgrad_ok(B, Ci, Co, Hi, Wi, 1) && dc_gemm1x1_wgrad_ok(B, Ci, Co, Hi, Wi, 1);
}
extern "C" int dc_conv1x1_stat_parts(int B, int Ci, int Co, int Hi, int Wi, int stride, int groups, int* ppg) {
    return dc_gemm1x1_stat_parts(B, Ci, Co, Hi, Wi, stride, groups, ppg);
}
extern "C" int dc_conv1x1_bwd_parts(int B, int Ci, int Co, int Hi, int Wi, int groups, int* ppg) {
    return dc_gemm1x1_bwd_parts(B, Ci, Co, Hi, Wi, 1, groups, ppg);
}
extern "C" int dc_conv1x1_fwd_bn(const float* x, const float* weight, float* y, int B, int Ci, int Co, int Hi, int Wi, int stride,
                                 const dc_bn_fold* bn, void* stream) {
    if (!bn_active(bn)) return dc_conv1x1_fwd(x, weight, y, B, Ci, Co, Hi, Wi, stride, stream);
    if (!dc_gemm1x1_fwd_ok(B, Ci, Co, Hi, Wi, stride)) return DC_EINVAL;
    return dc_gemm1x1_fwd(x, weight, nullptr, y, B, Ci, Co, Hi, Wi, stride, ACT_NONE, bn, stream);
}
extern "C" int dc_conv1x1_dgrad_bn(const float* gy, const float* weight, float* dx, const float* addend, int B, int Ci, int Co, int Hi,
                                   int Wi, int stride, const dc_bn_fold* bn, void* stream) {
    if (!bn || !bn->bwd_part) return dc_conv1x1_dgrad_add(gy, weight, dx, addend, B, Ci, Co, Hi, Wi, stride, stream);
    if (stride != 1 || !dc_gemm1x1_dgrad_ok(B, Ci, Co, Hi, Wi, stride)) return DC_EINVAL;
    return dc_gemm1x1_dgrad(gy, weight, dx, addend, nullptr, B, Ci, Co, Hi, Wi, stride, bn, stream);
}
extern "C" int dc_conv1x1_wgrad_bn(const float* x, const float* gy, float* dweight, void* ws, int B, int Ci, int Co, int Hi, int Wi,
                                   int stride, const dc_bn_fold* bn, void* stream) {
    if (!bn || !bn->in_scale) return dc_conv1x1_wgrad(x, gy, dweight, ws, B, Ci, Co, Hi, Wi, stride, stream);
    if (!dc_gemm1x1_wgrad_ok(B, Ci, Co, Hi, Wi, stride)) return DC_EINVAL;
    return dc_gemm1x1_wgrad(x, gy, dweight, ws, B, Ci, Co, Hi, Wi, stride, bn, stream);
}
