// Measurement hook of the convolution launchers (conv_prof.h): per kernel family, hipEvent pairs around the sampled launches and
// the flop / byte counts the launchers state for them.
#include "dc_common.h"
#include "conv_prof.h"

#include <vector>

namespace dc {

namespace {
struct ConvProf {
    std::vector<hipEvent_t> e0, e1;
    int used = 0;
    double flops = 0.0, exec = 0.0, bytes = 0.0;
};
ConvProf g_cprof[PROF_KINDS];
int g_cprof_cap = 0, g_cprof_every = 1;
unsigned g_cprof_seen[PROF_KINDS] = {};
}  // namespace

hipEvent_t conv_prof_begin(ConvProfKind kind, double algorithmic_flops, double executed_flops, double algorithmic_bytes, hipStream_t st) {
    ConvProf& d = g_cprof[kind];
    if (g_cprof_cap == 0 || (g_cprof_seen[kind]++ % (unsigned)g_cprof_every) != 0 || d.used >= g_cprof_cap) return nullptr;
    d.flops += algorithmic_flops; d.exec += executed_flops; d.bytes += algorithmic_bytes;
    (void)hipEventRecord(d.e0[d.used], st);
    return d.e1[d.used++];
}
void conv_prof_end(hipEvent_t e, hipStream_t st) {
    if (e) (void)hipEventRecord(e, st);
}

}  // namespace dc

using namespace dc;

extern "C" int dc_conv_profile_enable(int max_launches, int every) {
    g_cprof_every = every > 0 ? every : 1;
    for (auto& v : g_cprof_seen) v = 0;
    for (auto& d : g_cprof) {
        for (auto e : d.e0) (void)hipEventDestroy(e);
        for (auto e : d.e1) (void)hipEventDestroy(e);
        d.e0.clear(); d.e1.clear(); d.used = 0; d.flops = d.exec = d.bytes = 0.0;
    }
    g_cprof_cap = 0;
    if (max_launches <= 0) return DC_OK;
    for (auto& d : g_cprof) {
        d.e0.resize(max_launches); d.e1.resize(max_launches);
        for (int i = 0; i < max_launches; ++i)
            if (hipEventCreate(&d.e0[i]) != hipSuccess || hipEventCreate(&d.e1[i]) != hipSuccess) return DC_ELAUNCH;
    }
    g_cprof_cap = max_launches;
    return DC_OK;
}

extern "C" int dc_conv_profile_collect(int kind, double* ms, double* algorithmic_flops, double* executed_flops,
                                       double* algorithmic_bytes, int* launches) {
    if (kind < 0 || kind >= PROF_KINDS) return DC_EINVAL;
    ConvProf& d = g_cprof[kind];
    double tot = 0.0;
    for (int i = 0; i < d.used; ++i) {
        float t = 0.f;
        if (hipEventSynchronize(d.e1[i]) != hipSuccess || hipEventElapsedTime(&t, d.e0[i], d.e1[i]) != hipSuccess) return DC_ELAUNCH;
        tot += t;
    }
    if (ms) *ms = tot;
    if (algorithmic_flops) *algorithmic_flops = d.flops;
    if (executed_flops) *executed_flops = d.exec;
    if (algorithmic_bytes) *algorithmic_bytes = d.bytes;
    if (launches) *launches = d.used;
    d.used = 0; d.flops = d.exec = d.bytes = 0.0;
    return DC_OK;
}
