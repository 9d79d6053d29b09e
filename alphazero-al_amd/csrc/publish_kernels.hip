// publish_kernels.hip - the learner's float32 parameters become a live evaluator's weights (az_nn_publish_dev in az_nn.h):
// the layout function az_nn.h documents tensor by tensor - casts to bf16, the position table, OIHW -> OHWI convolution
// weights, the folded stem's two tables, three float32 scalars - as ONE launch that writes the arrays an
// az_nn_model_weights names, in place.
//
//   k_publish   a job table in the kernel arguments (destination, source, kind, count; the first workgroup of every job).
//               A workgroup finds its job from its index and does one piece of it:
//     SMALL     a tensor of at most a few hundred elements: bf16(src[i]) with 2-byte stores, one workgroup.
//     CAST      2048 elements per workgroup: float32 in with 4-byte loads in element order (the sources are only 4-byte
//               aligned), through LDS, out as one 16-byte store of eight bf16 per lane.
//     POS       pos[cell][c] = bf16(pos_emb[orbit(cell)][c]): one 16-byte store per eight channels.
//     CONV      workgroup o: W[o] (c_in * 9 floats, contiguous) into LDS, out as [tap][c] rows of 16-byte stores.
//     FOLD      workgroup o: W[o] rounded to bf16 and the two embedding tables into LDS; lanes 0 .. 47 of the first
//               wavefront own column o of pmap (one cell each, rows 42 .. 47 zeros), lanes 0 .. 31 of the second T[o][k],
//               which four lanes then scatter as high and low halves into the fragment order.  Workgroups 0 .. 3 also
//               write the zero columns 64 .. 67 of pmap.
//     SCALARS   the three float32 biases into the caller's slot.
//   Every job reads SOURCES only (the fold rounds W itself, it never reads the stem_w another workgroup is writing), so no
//   workgroup waits for another, and every destination byte is written by exactly one lane.  No atomics, no scratch; the
//   stores are plain vector stores.  About 1 MB moves: the launch is what it costs.
//
// The order of every float32 sum is part of the contract (az_nn.h): each step is one multiply and one add (the build has
// -ffp-contract=off and nothing here calls fmaf), so that tests/publish_ref.py reproduces the bytes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "az_nn.h"
#include "nn_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int CELLS = 42, COLS = 7, ROWS = 6, EMB = 32, CH = 64, TAPS = 9;
constexpr int ORBITS = 24;                          // rows of pos_emb
constexpr int CHUNK = 8 * THREADS;                  // elements of a CAST workgroup
constexpr int PMAP_ROWS = 48, PMAP_COLS = 68;
constexpr int MAX_JOBS = 64;                        // 60 with eight blocks and the folded stem
enum Kind : int32_t { SMALL = 0, CAST = 1, POS = 2, CONV = 3, FOLD = 4, SCALARS = 5 };

struct Job {
    void *dst;
    const float *src;
    int32_t kind;
    int32_t count;              // elements; CONV: c_in
};

struct PublishArgs {
    Job job[MAX_JOBS];
    int32_t first[MAX_JOBS + 1];            // job j owns workgroups first[j] .. first[j + 1] - 1
    int32_t n_jobs;
    const float *piece_emb, *pos_emb, *stem_w, *stem_b;     // what FOLD reads
    uint16_t *frag;
    float *pmap;
    const float *scalar[3];
    float *scalars;
};

__device__ __forceinline__ int orbit(int cell) { const int c = cell % COLS; return 4 * (cell / COLS) + (c < COLS - 1 - c ? c : COLS - 1 - c); }
__device__ __forceinline__ uint16_t bf16_bits(float v) { return static_cast<uint16_t>(pack2(v, 0.0f) & 0xffffu); }
__device__ __forceinline__ float bf16_round(float v) { return bf_lo(pack2(v, 0.0f)); }
__device__ __forceinline__ V8 pack8(const float *v)
{
    return V8{{pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])}};
}

__global__ void __launch_bounds__(THREADS) k_publish(const PublishArgs a)
{
    __shared__ float buf[CHUNK];                    // CAST: a chunk; CONV, FOLD: W[o] (at most 64 * 9 floats)
    __shared__ float pe[ORBITS * EMB];              // FOLD: pos_emb
    __shared__ float em[2 * EMB];                   // FOLD: piece_emb
    __shared__ float trow[EMB];                     // FOLD: T[o][0 .. 31]
    const int t = threadIdx.x;
    const int wg = blockIdx.x;
    int j = 0;
    while (j + 1 < a.n_jobs && wg >= a.first[j + 1]) ++j;
    const int part = wg - a.first[j];               // which workgroup of the job
    const Job job = a.job[j];

    if (job.kind == SMALL) {
        uint16_t *dst = static_cast<uint16_t *>(job.dst);
        for (int i = t; i < job.count; i += THREADS) dst[i] = bf16_bits(job.src[i]);
    } else if (job.kind == CAST) {
        const int base = part * CHUNK;
        const int n = job.count - base < CHUNK ? job.count - base : CHUNK;          // a multiple of 8
        for (int i = t; i < n; i += THREADS) buf[i] = job.src[base + i];
        __syncthreads();
        if (8 * t < n) *reinterpret_cast<V8 *>(static_cast<uint16_t *>(job.dst) + base + 8 * t) = pack8(buf + 8 * t);
    } else if (job.kind == POS) {
        if (t < CELLS * EMB / 8) {
            const int cell = t / (EMB / 8), c0 = 8 * (t % (EMB / 8));
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = job.src[orbit(cell) * EMB + c0 + k];
            *reinterpret_cast<V8 *>(static_cast<uint16_t *>(job.dst) + cell * EMB + c0) = pack8(v);
        }
    } else if (job.kind == CONV) {
        const int c_in = job.count, o = part;
        const float *w = job.src + o * c_in * TAPS;
        for (int i = t; i < c_in * TAPS; i += THREADS) buf[i] = w[i];
        __syncthreads();
        const int per_tap = c_in / 8;
        for (int i = t; i < TAPS * per_tap; i += THREADS) {
            const int tap = i / per_tap, c0 = 8 * (i % per_tap);
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = buf[(c0 + k) * TAPS + tap];
            *reinterpret_cast<V8 *>(static_cast<uint16_t *>(job.dst) + (o * TAPS + tap) * c_in + c0) = pack8(v);
        }
    } else if (job.kind == FOLD) {
        const int o = part;
        for (int i = t; i < EMB * TAPS; i += THREADS) buf[i] = bf16_round(a.stem_w[o * EMB * TAPS + i]);
        for (int i = t; i < ORBITS * EMB; i += THREADS) pe[i] = a.pos_emb[i];
        if (t < 2 * EMB) em[t] = a.piece_emb[t];
        __syncthreads();
        if (t < PMAP_ROWS) {
            // pmap[cell][o]: taps ascending (ky, then kx), c ascending inside a tap, one running sum, the bias last
            float acc = 0.0f;
            if (t < CELLS) {
                const int y = t / COLS, x = t % COLS;
                for (int tap = 0; tap < TAPS; ++tap) {
                    const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
                    if (yy < 0 || yy >= ROWS || xx < 0 || xx >= COLS) continue;
                    const float *p = pe + orbit(yy * COLS + xx) * EMB;
                    for (int c = 0; c < EMB; ++c) {
                        const float prod = buf[c * TAPS + tap] * p[c];
                        acc = acc + prod;
                    }
                }
                acc = acc + bf16_round(a.stem_b[o]);
            }
            a.pmap[t * PMAP_COLS + o] = acc;
            if (o < PMAP_COLS - CH) a.pmap[t * PMAP_COLS + CH + o] = 0.0f;
        } else if (t >= 64 && t < 64 + EMB) {
            // T[o][k], k = 2 tap + plane: c ascending from 0; k >= 18 zero
            const int k = t - 64;
            float acc = 0.0f;
            if (k < 2 * TAPS) {
                const int tap = k >> 1, plane = k & 1;
                for (int c = 0; c < EMB; ++c) {
                    const float prod = buf[c * TAPS + tap] * em[plane * EMB + c];
                    acc = acc + prod;
                }
            }
            trow[k] = acc;
        }
        __syncthreads();
        if (t < 8) {
            // channel o is row r of channel tile ti (az_nn.h): lanes 16 g + r hold its k = 8 g .. 8 g + 7
            const int g = t & 3, half = t >> 2;                 // half 0: the high parts, 1: the low parts
            const int ti = 2 * (o / 32) + (o % 8) / 4, r = 4 * ((o % 32) / 8) + o % 4;
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float full = trow[8 * g + k], hi = bf16_round(full);
                v[k] = half == 0 ? hi : full - hi;
            }
            *reinterpret_cast<V8 *>(a.frag + ((half * 4 + ti) * 64 + 16 * g + r) * 8) = pack8(v);
        }
    } else if (job.kind == SCALARS) {
        if (t < 3) a.scalars[t] = *a.scalar[t];
    }
}

bool aligned_to(const void *p, uintptr_t to) { return p != nullptr && reinterpret_cast<uintptr_t>(p) % to == 0; }

}  // namespace

extern "C" int az_nn_publish_dev(const az_nn_publish_src *src, const az_nn_model_weights *dst, float *scalars_dev, void *stream)
{
    if (src == nullptr || dst == nullptr) return 1;
    if (src->n_blocks < 1 || src->n_blocks > AZ_NN_MAX_BLOCKS || src->n_blocks != dst->n_blocks) return 1;
    if ((dst->stem_frag == nullptr) != (dst->stem_pmap == nullptr)) return 1;
    if (!aligned_to(scalars_dev, 4)) return 1;
    const bool fold = dst->stem_frag != nullptr;
    const int nb = src->n_blocks;

    PublishArgs a{};
    int n = 0, wgs = 0;
    bool ok = true;
    // a destination's alignment: 16 bytes where its stores are 16 bytes, else its element's
    auto add = [&](void *d, const float *s, int32_t kind, int32_t count, int n_wg, uintptr_t dst_align) {
        ok = ok && aligned_to(s, 4) && aligned_to(d, dst_align) && n < MAX_JOBS;
        if (!ok) return;
        a.job[n] = Job{d, s, kind, count};
        a.first[n] = wgs;
        wgs += n_wg;
        ++n;
    };
    auto w = [](const void *p) { return const_cast<void *>(p); };
    auto small = [&](const void *d, const float *s, int count) { add(w(d), s, SMALL, count, 1, 2); };
    auto cast = [&](const void *d, const float *s, int count) { add(w(d), s, CAST, count, (count + CHUNK - 1) / CHUNK, 16); };
    const az_nn_heads_weights &h = dst->heads;

    small(dst->emb_own, src->piece_emb, EMB);
    small(dst->emb_opp, src->piece_emb != nullptr ? src->piece_emb + EMB : nullptr, EMB);
    add(w(dst->pos), src->pos_emb, POS, CELLS * EMB, 1, 16);
    add(w(dst->stem_w), src->stem_conv_weight, CONV, EMB, CH, 16);
    small(dst->stem_b, src->stem_conv_bias, CH);
    for (int k = 0; k < nb; ++k) {
        add(w(dst->block_w[k]), src->block_conv_weight[k], CONV, CH, CH, 16);
        small(dst->block_b[k], src->block_conv_bias[k], CH);
        small(dst->block_gamma[k], src->block_norm_weight[k], CH);
        small(dst->block_beta[k], src->block_norm_bias[k], CH);
    }
    small(dst->pre_w, src->prenorm_weight, CH);
    cast(dst->qkvg_w, src->qkv_weight, 3 * CH * CH);           // a null qkvg_w ends here: the next line's sum is not null
    cast(static_cast<const uint16_t *>(dst->qkvg_w) + 3 * CH * CH, src->gate_weight, 4 * CH);
    cast(dst->o_w, src->o_weight, CH * CH);
    small(dst->qn_w, src->q_norm_weight, 16);
    small(dst->kn_w, src->k_norm_weight, 16);
    small(h.p_norm, src->policy_norm_weight, CH);
    small(h.p_gate_w, src->row_gate_weight, CH);
    cast(h.p_fc_w, src->policy_fc_weight, CH * CH);
    small(h.p_fc_b, src->policy_fc_bias, CH);
    small(h.p_out_w, src->policy_out_weight, CH);
    small(h.d_pool_norm, src->pool_norm_weight, CH);
    cast(h.d_pool_w, src->pool_fc_weight, CH * CH);
    small(h.d_pool_b, src->pool_fc_bias, CH);
    small(h.d_norm, src->norm_weight, CH);
    cast(h.d_fc_w, src->fc_weight, CH * CH);
    small(h.d_fc_b, src->fc_bias, CH);
    small(h.d_out_norm, src->out_norm_weight, CH);
    small(h.d_val_w, src->value_out_weight, 3 * CH);
    small(h.d_val_b, src->value_out_bias, 3);
    small(h.d_aux_w, src->aux_out_weight, CH);
    if (fold) {
        add(w(dst->stem_frag), src->stem_conv_weight, FOLD, 0, CH, 16);
        ok = ok && aligned_to(dst->stem_pmap, 4);
    }
    add(scalars_dev, src->row_gate_bias, SCALARS, 3, 1, 4);
    ok = ok && aligned_to(src->policy_out_bias, 4) && aligned_to(src->aux_out_bias, 4);
    if (!ok) return 1;
    a.first[n] = wgs;
    a.n_jobs = n;
    a.piece_emb = src->piece_emb; a.pos_emb = src->pos_emb; a.stem_w = src->stem_conv_weight; a.stem_b = src->stem_conv_bias;
    a.frag = static_cast<uint16_t *>(w(dst->stem_frag));
    a.pmap = const_cast<float *>(dst->stem_pmap);
    a.scalar[0] = src->row_gate_bias; a.scalar[1] = src->policy_out_bias; a.scalar[2] = src->aux_out_bias;
    a.scalars = scalars_dev;
    hipLaunchKernelGGL(k_publish, dim3(static_cast<unsigned>(wgs)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
