// The per-step prepared-weight cache behind dc_wino_cache_* (include/depthcore.h): registered weights, their prepared variants
// (Winograd U, the bf16 direct kernels' packed weights, the split 1x1 weights) and the one batched launch that refreshes them.
#include "dc_common.h"
#include "conv_bf16.h"
#include "gemm1x1_x3.h"
#include "weight_cache.h"

#include <mutex>
#include <vector>

namespace dc {

// Every registered weight of a model in ONE launch (dc_wino_cache_refresh): `table` holds one descriptor per (weight,
// dgrad, MT) variant with the first block of its range; a block finds its descriptor by binary search.
struct WinoWDesc {
    const float* w; float* uhat;
    int Co, Ci, MT, Mp, Kp, dgrad, block0, kind;      // kind 1: the bf16 direct kernels' prepared weights (Mp = m-blocks, Kp = chunks)
};
__global__ __launch_bounds__(256) void wino_weights_batched_kernel(const WinoWDesc* __restrict__ table, const int* __restrict__ blk2desc, int WK) {
    // (a per-block binary search over the table -- eight dependent global loads in front of every block -- made this launch
    // 310 us for 0.5 GB; the host uploads the block -> descriptor map next to the table instead)
    const WinoWDesc d = table[blk2desc[blockIdx.x]];
    const int idx = ((int)blockIdx.x - d.block0) * 256 + threadIdx.x;
    if (d.kind == 1) { c3b_wprep_item(d.w, reinterpret_cast<uint4*>(d.uhat), idx, d.Co, d.Ci, d.dgrad, d.MT, d.Mp, d.Kp); return; }
    if (d.kind == 2) {       // split-operand 1x1 GEMMs: (Mp, Kp) = (padded rows, reduction extent) of this direction
        g1x3_prep_item(d.w, reinterpret_cast<unsigned short*>(d.uhat), idx, d.dgrad, d.dgrad ? d.Ci : d.Co, d.Mp, d.Kp);
        return;
    }
    if (d.dgrad) wino_weight_one<true>(d.w, d.uhat, idx, d.Co, d.Ci, d.MT, d.Mp, d.Kp, WK);
    else wino_weight_one<false>(d.w, d.uhat, idx, d.Co, d.Ci, d.MT, d.Mp, d.Kp, WK);
}

// ---- transformed-weight cache ---------------------------------------------------------------------------------------
// A training step uses every convolution weight twice (forward: G g G^T, data gradient: the same of the rotated,
// transposed filter) and, in the sequence models, once per frame; the weights only change in the optimiser step.  The
// host registers the weights of a model once (dc_wino_cache_register), calls dc_wino_cache_refresh at the start of a
// step -- ONE launch that transforms every variant seen so far instead of one 8 us launch in front of every convolution
// -- and dc_wino_cache_invalidate when the step's backward is done.  Between the two, wino_launch takes U from the
// cache; a variant (dgrad, MT) it has not met yet is transformed in place as before and joins the next refresh.
struct WcVariant { int dgrad, MT, Mp, Kp; float* buf; bool fresh, in_table; int kind; };     // kind 0 Winograd U, 1 bf16 prepared weights, 2 split 1x1 weights
struct WcEntry { const float* w; int Ci, Co, owner; std::vector<WcVariant> v; };
// One descriptor table PER OWNER (= per model / Trainer).  A refresh transforms -- and a captured hipGraph replays the
// transform of -- the owner's own weights only, which the owner keeps alive; weights of another owner never enter its
// table.  (Round 3 had one table for the whole process: a graph captured, or a refresh skipped because the stream was
// capturing, while the table still named the weights of a model that had since been collected read freed memory -- a GPU
// page fault, which the HSA runtime turns into abort() of the process.  See DESIGN.md "The r3s abort".)
struct WcOwner {
    int id;
    bool valid = false, dirty = true;
    WinoWDesc* table = nullptr;
    int* b2d = nullptr;
    int table_n = 0, blocks = 0;
};
static std::mutex g_wc_mu;
static std::vector<WcEntry> g_wc;
static std::vector<WcOwner> g_wc_owners;
static int g_wc_next_owner = 1;
// Device buffers a captured hipGraph may still name in its kernel arguments (descriptor tables that were outgrown, the
// variant buffers of unregistered weights): parked here, released only by dc_wino_cache_clear().
static std::vector<void*> g_wc_retired;

static bool wc_capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
    return cs != hipStreamCaptureStatusNone;
}
static WcOwner* wc_owner(int id) {
    for (auto& o : g_wc_owners)
        if (o.id == id) return &o;
    return nullptr;
}

// -> cached U for this launch, or nullptr (then the caller transforms into its workspace).  Nothing is allocated while
// `st` is being captured (hipMalloc is illegal there): an unseen variant is then transformed per launch, as before.
static inline size_t wc_variant_bytes(int kind, int MT, int Mp, int Kp) {
    if (kind == 2) return (size_t)Mp * Kp * 3 * 2 + 256;
    return kind == 1 ? (size_t)Mp * Kp * 36 * MT * 16 : (size_t)Mp * Kp * 16 * sizeof(float);
}
static inline int wc_variant_blocks(int kind, int MT, int Mp, int Kp) {
    if (kind == 2) return ceil_div(Mp * (Kp / 4), 256);
    return kind == 1 ? ceil_div(Mp * Kp * 36 * MT, 256) : wino_wblocks(Mp, Kp);
}
static const float* wc_lookup_kind(int kind, const float* w, int Ci, int Co, bool dgrad, int MT, int Mp, int Kp, hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_wc_mu);
    for (auto& e : g_wc) {
        if (e.w != w) continue;
        if (e.Ci != Ci || e.Co != Co) return nullptr;
        WcOwner* o = wc_owner(e.owner);
        if (!o) return nullptr;
        for (auto& v : e.v)
            if (v.kind == kind && v.dgrad == (int)dgrad && v.MT == MT) return (o->valid && v.fresh) ? v.buf : nullptr;
        if (wc_capturing(st)) return nullptr;
        WcVariant v{(int)dgrad, MT, Mp, Kp, nullptr, false, false, kind};
        if (hipMalloc((void**)&v.buf, wc_variant_bytes(kind, MT, Mp, Kp)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        e.v.push_back(v);
        o->dirty = true;
        return nullptr;
    }
    return nullptr;
}
const float* wc_lookup(const float* w, int Ci, int Co, bool dgrad, int MT, int Mp, int Kp, hipStream_t st) {
    return wc_lookup_kind(0, w, Ci, Co, dgrad, MT, Mp, Kp, st);
}
const void* wc_lookup_c3b(const float* w, int Ci, int Co, int dgrad, int MT, int nmblk, int nchunks, hipStream_t st) {
    return wc_lookup_kind(1, w, Ci, Co, dgrad != 0, MT, nmblk, nchunks, st);
}
const void* wc_lookup_x3(const float* w, int Ci, int Co, int tr, int Mp, int K, hipStream_t st) {
    return wc_lookup_kind(2, w, Ci, Co, tr != 0, 0, Mp, K, st);
}

}  // namespace dc

using namespace dc;

extern "C" int dc_wino_cache_new_owner(void) {
    std::lock_guard<std::mutex> lk(g_wc_mu);
    WcOwner o;
    o.id = g_wc_next_owner++;
    g_wc_owners.push_back(o);
    return o.id;
}

extern "C" int dc_wino_cache_register(int owner, const float* weight, int Ci, int Co) {
    if (!weight || Ci <= 0 || Co <= 0) return DC_EINVAL;
    std::lock_guard<std::mutex> lk(g_wc_mu);
    WcOwner* o = wc_owner(owner);
    if (!o) return DC_EINVAL;
    for (auto& e : g_wc)
        if (e.w == weight) return (e.Ci == Ci && e.Co == Co && e.owner == owner) ? DC_OK : DC_EINVAL;
    g_wc.push_back(WcEntry{weight, Ci, Co, owner, {}});
    o->dirty = true;
    return DC_OK;
}

// Forget an owner and every weight it registered.  Its tables and variant buffers are parked, not freed: a captured
// hipGraph of the owner may still name them.
extern "C" int dc_wino_cache_release_owner(int owner) {
    std::lock_guard<std::mutex> lk(g_wc_mu);
    for (size_t i = 0; i < g_wc.size();) {
        if (g_wc[i].owner == owner) {
            for (auto& v : g_wc[i].v)
                if (v.buf) g_wc_retired.push_back(v.buf);
            g_wc.erase(g_wc.begin() + i);
        } else {
            ++i;
        }
    }
    for (size_t i = 0; i < g_wc_owners.size(); ++i)
        if (g_wc_owners[i].id == owner) {
            if (g_wc_owners[i].table) g_wc_retired.push_back(g_wc_owners[i].table);
            if (g_wc_owners[i].b2d) g_wc_retired.push_back(g_wc_owners[i].b2d);
            g_wc_owners.erase(g_wc_owners.begin() + i);
            break;
        }
    return DC_OK;
}

extern "C" int dc_wino_cache_refresh(int owner, void* stream) {
    std::lock_guard<std::mutex> lk(g_wc_mu);
    hipStream_t st = (hipStream_t)stream;
    WcOwner* o = wc_owner(owner);
    if (!o) return DC_EINVAL;
    // The descriptor upload allocates, synchronises and copies: none of it is legal on a capturing stream.  A capture that
    // meets a dirty registry replays the owner's table as it stands (variants outside it keep transforming per launch);
    // every weight the table names belongs to this owner and lives as long as it does.
    if (o->dirty && !wc_capturing(st)) {
        std::vector<WinoWDesc> host;
        std::vector<int> b2d;
        int blocks = 0;
        for (auto& e : g_wc) {
            if (e.owner != owner) continue;
            for (auto& v : e.v) {
                const int nb = wc_variant_blocks(v.kind, v.MT, v.Mp, v.Kp);
                b2d.insert(b2d.end(), nb, (int)host.size());
                host.push_back(WinoWDesc{e.w, v.buf, e.Co, e.Ci, v.MT, v.Mp, v.Kp, v.dgrad, blocks, v.kind});
                blocks += nb;
            }
        }
        // A rebuilt table goes to fresh memory and the old one is retired, not freed or rewritten: a captured graph holds
        // the old address and block count and must keep seeing the old contents.
        if (o->b2d) g_wc_retired.push_back(o->b2d);
        if (o->table) g_wc_retired.push_back(o->table);
        o->b2d = nullptr; o->table = nullptr; o->table_n = o->blocks = 0;
        if (blocks > 0 && hipMalloc((void**)&o->b2d, sizeof(int) * blocks) != hipSuccess) { o->b2d = nullptr; return DC_ELAUNCH; }
        if (!host.empty() && hipMalloc((void**)&o->table, sizeof(WinoWDesc) * host.size()) != hipSuccess) { o->table = nullptr; return DC_ELAUNCH; }
        // synchronous upload (the descriptor list only changes while the variants of a model are still being met)
        if (!host.empty() && hipStreamSynchronize(st) != hipSuccess) return DC_ELAUNCH;
        if (!host.empty() && hipMemcpy(o->table, host.data(), sizeof(WinoWDesc) * host.size(), hipMemcpyHostToDevice) != hipSuccess) return DC_ELAUNCH;
        if (!b2d.empty() && hipMemcpy(o->b2d, b2d.data(), sizeof(int) * b2d.size(), hipMemcpyHostToDevice) != hipSuccess) return DC_ELAUNCH;
        o->table_n = (int)host.size(); o->blocks = blocks; o->dirty = false;
        for (auto& e : g_wc)
            if (e.owner == owner)
                for (auto& v : e.v) v.in_table = true;
    }
    if (o->table_n > 0 && o->blocks > 0) {
        hipLaunchKernelGGL(wino_weights_batched_kernel, dim3(o->blocks), dim3(256), 0, st, (const WinoWDesc*)o->table, (const int*)o->b2d, PSK);
        DC_CHECK_LAUNCH();
    }
    for (auto& e : g_wc)
        if (e.owner == owner)
            for (auto& v : e.v) v.fresh = v.in_table;
    o->valid = true;
    return DC_OK;
}

extern "C" int dc_wino_cache_invalidate(int owner) {
    std::lock_guard<std::mutex> lk(g_wc_mu);
    WcOwner* o = wc_owner(owner);
    if (!o) return DC_EINVAL;
    o->valid = false;
    return DC_OK;
}

extern "C" int dc_wino_cache_clear(void) {
    std::lock_guard<std::mutex> lk(g_wc_mu);
    int rc = DC_OK;
    if (hipDeviceSynchronize() != hipSuccess) rc = DC_ELAUNCH;
    for (auto& e : g_wc)
        for (auto& v : e.v)
            if (v.buf && hipFree(v.buf) != hipSuccess) rc = DC_ELAUNCH;
    g_wc.clear();
    for (void* q : g_wc_retired)
        if (hipFree(q) != hipSuccess) rc = DC_ELAUNCH;
    g_wc_retired.clear();
    for (auto& o : g_wc_owners) {
        if (o.table && hipFree(o.table) != hipSuccess) rc = DC_ELAUNCH;
        if (o.b2d && hipFree(o.b2d) != hipSuccess) rc = DC_ELAUNCH;
    }
    g_wc_owners.clear();
    return rc;
}

extern "C" int dc_wino_cache_variants(void) {
    std::lock_guard<std::mutex> lk(g_wc_mu);
    int n = 0;
    for (auto& e : g_wc) n += (int)e.v.size();
    return n;
}
