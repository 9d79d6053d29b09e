// dev_rng.h - the counter-based generator of the dev_* entry points, shared by the search kernels
// (kernels.hip: symmetry ids, re-rooting noise, random playouts; backup_kernels.hip: Dirichlet noise of root
// expansions) and the self-play driver's move
// sampler (selfplay_kernels.hip).  A stream is named by (seed, call, a, b): the engine's seed, a
// counter that moves per use, an index (tree, leaf, game) and a small constant per purpose - streams
// in use: b = 3 playouts, 7 symmetry ids, 16.. and 128.. root noise, SP_STREAM the driver's moves,
// REPLAY_STREAM the replay sampler's ring indices (replay_kernels.hip), MATCH_STREAM the evaluation-match
// driver's moves (match_kernels.hip), LEARN_STREAM + t (t = 0 .. 10) the learner's dropout draws of tensor t
// (learn_driver.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace az {

__device__ __forceinline__ uint64_t mix64(uint64_t x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

struct DevRng {
    uint64_t s;
    __device__ DevRng(uint64_t seed, uint64_t call, uint64_t a, uint64_t b)
        : s(mix64(seed ^ mix64(call + 0x9E3779B97F4A7C15ull * (a + 1)) ^ (b << 32))) {}
    __device__ uint32_t next() { s += 0x9E3779B97F4A7C15ull; return static_cast<uint32_t>(mix64(s) >> 32); }
    __device__ float uniform() { return (static_cast<float>(next() >> 8) + 0.5f) * (1.0f / 16777216.0f); }
    __device__ float normal()
    {
        const float u1 = uniform(), u2 = uniform();
        return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530718f * u2);
    }
    __device__ float gamma(float alpha)   // Marsaglia-Tsang, boosted for alpha < 1
    {
        const float a = alpha < 1.0f ? alpha + 1.0f : alpha;
        const float d = a - 1.0f / 3.0f, c = 1.0f / sqrtf(9.0f * d);
        float v = 1.0f, x, u;
        for (int it = 0; it < 64; ++it) {
            x = normal();
            v = 1.0f + c * x;
            if (v <= 0.0f) continue;
            v = v * v * v;
            u = uniform();
            if (u < 1.0f - 0.0331f * x * x * x * x) break;
            if (logf(u) < 0.5f * x * x + d * (1.0f - v + logf(v))) break;
        }
        float g = d * v;
        if (alpha < 1.0f) g *= powf(uniform(), 1.0f / alpha);
        return g;
    }
};

constexpr uint64_t SP_STREAM = 0x5350;       // the self-play driver's move draws
constexpr uint64_t REPLAY_STREAM = 0x5242;   // ring indices of a training sample (k_replay_indices)
constexpr uint64_t MATCH_STREAM = 0x4D54;    // the evaluation-match driver's move draws (k_match_ply)
constexpr uint64_t LEARN_STREAM = 0x4C52;    // + tensor id: the learner's dropout draws (k_learn_keep), 0x4C52 .. 0x4C5C

}  // namespace az
