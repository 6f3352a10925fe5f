// The per-element expressions of the ConvLSTM v8 passes and their launch shape, stated once for the training forms (lstm.hip),
// the inference step (lstm_infer.hip) and the ConvGRU v10 hand-over (gru_c2f.hip); the hand-over's item walk, which the three
// share, is c2f_dev.h.  sigmoid and tanh are the accurate expf / tanhf (not __expf): the states are carried over the frames of
// a sequence.
#pragma once
#include "dc_common.h"

#include <algorithm>
#include <initializer_list>

namespace dc {

constexpr int LSTM_BLOCK = 256;     // threads per block; a float4 body block covers 1024 floats of a batch item

__device__ __forceinline__ float lstm_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

struct LstmFwd { float h, c; };
__device__ __forceinline__ LstmFwd lstm_fwd1(float ci, float cf, float co, float cg, float c) {
    LstmFwd r;
    r.c = lstm_sigmoid(cf) * c + lstm_sigmoid(ci) * tanhf(cg);          // rnn.py:71-76
    r.h = lstm_sigmoid(co) * tanhf(r.c);                                // rnn.py:77
    return r;
}

// PixelShuffle(2): up[b, q, 2y + i, 2x + j] = tanh(pre[b, 4q + 2i + j, y, x]).
__device__ __forceinline__ float handover_pre(float a, float hp, float hn) { return fmaxf(a + (hp + hn) * 0.5f, 0.f); }
// d(pre pre-ReLU) from the two consumers of pre: the ReLU's mask, the tanh recomputed from pre
__device__ __forceinline__ float handover_d(float pre, float gp, float gu) {
    const float t = tanhf(pre);
    return pre > 0.f ? gp + gu * (1.f - t * t) : 0.f;
}

static inline unsigned lstm_grid(size_t work) { return (unsigned)std::min<size_t>((work + LSTM_BLOCK - 1) / LSTM_BLOCK, 4096); }

static inline bool all16(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if ((size_t)p & 15) return false;
    return true;
}

}  // namespace dc
