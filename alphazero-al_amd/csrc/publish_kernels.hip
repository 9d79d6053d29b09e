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

// ---------------------------------------------------------------------------------------------------------------------
// The Othello network's (az_nn_othello_publish_dev in az_nn.h): the same recipe - a job table in the kernel arguments, a
// workgroup finds its job from its index, every job reads SOURCES only.
//
//   k_publish_othello
//     O_EMBED   the (64 cells x 4 kinds, 32) table: one float32 add per element, one 16-byte store per eight channels.
//     O_CONV    workgroup (tile, kc) of a [rows][c_in][3][3] weight: its 16 rows of 288 contiguous floats in element order
//               into LDS (rows padded to 289 floats), out as nine runs of 1 KB, one per tap: 64 lanes x one 16-byte store,
//               each lane's eight j packed from LDS.  128 workgroups for a 256-channel layer, 16 for the stem, 8 for the
//               bottleneck (one tile, rows 8 .. 15 zeros).
//     O_BN      one BatchNorm as scale / shift, one workgroup; it takes two table entries (weight, var -> scale; bias,
//               mean -> shift).  `pad16`: entries count .. 15 are 1.0f / 0.0f (the bottleneck's).
//     O_TRANS   a 64 x 64 tile of the 512 x 512 transpose through LDS: loads and stores both in element order.
//     O_PERM16  eight rows of a_fc_w16: 8 x 512 floats into LDS, out as [cell][c] bf16, one 16-byte store per cell.
//     O_VCONV   v_conv_w[ci * 9 + k][co] = W[co][ci][k] (576 floats);  O_COPY a float32 copy;  O_BF16 a bf16 cast of a small
//               tensor;  O_SCALARS the three biases (two table entries).
//   No atomics, no scratch, plain vector stores; every destination byte is written by exactly one lane.
//
// The BatchNorm affine is four float32 operations, each correctly rounded: the build has -ffp-contract=off and no fast-math
// flag, and sqrtf and / are correctly rounded under hipcc's defaults.

namespace {

constexpr int O_CH = 256, O_EMB = 32, O_CELLS = 64, O_ROW = 32 * TAPS;          // 288 floats of one output row and kc chunk
constexpr int O_ROW_PAD = O_ROW + 1;                                             // LDS stride of a row: odd, so that the 16 rows of a tap spread over the banks
constexpr int O_TILE = 64, O_TILE_PAD = O_TILE + 1;                              // the transpose's tile
constexpr int O_FC = 512, O_PERM_ROWS = 8;
constexpr int O_LDS = 16 * O_ROW_PAD;                                            // 4624 floats: >= 64 * 65 and >= 8 * 512
constexpr int O_MAX_JOBS = 100;                                                  // 16 convolutions, 34 BatchNorms at two entries, 16 more
static_assert(O_LDS >= O_TILE * O_TILE_PAD && O_LDS >= O_PERM_ROWS * O_FC, "one LDS buffer serves every job kind");
enum OKind : int32_t { O_EMBED = 0, O_CONV = 1, O_BN = 2, O_TRANS = 3, O_PERM16 = 4, O_VCONV = 5, O_COPY = 6, O_BF16 = 7, O_SCALARS = 8,
                       O_SECOND = 9 };

struct OJob {
    void *dst;
    const float *src, *aux;     // O_EMBED: pos_emb, piece_emb (the entry behind it: legal_emb); O_BN: weight, var / bias, mean
    int32_t kind;
    int32_t count;              // elements; O_CONV: c_in | rows << 16 | tiles << 24; O_BN: channels | pad16 << 16
};
static_assert(sizeof(OJob) == 32, "OJob");

struct OthelloPublishArgs {
    OJob job[O_MAX_JOBS];
    int32_t first[O_MAX_JOBS + 1];          // job j owns workgroups first[j] .. first[j + 1] - 1
    int32_t n_jobs;
    float bn_eps;
};
static_assert(sizeof(OthelloPublishArgs) <= 4096, "the job table travels in the kernel arguments");

// the reference's 64-entry orbit table (Othello/Network.py _ORBIT_MAP) as its closed form: the octant's triangle a <= b <= 3
// numbered row by row
__device__ __forceinline__ int othello_orbit(int cell)
{
    const int r = cell >> 3, c = cell & 7;
    const int fr = r < 7 - r ? r : 7 - r, fc = c < 7 - c ? c : 7 - c;
    const int a = fr < fc ? fr : fc, b = fr < fc ? fc : fr;
    return (a == 0 ? 0 : a == 1 ? 4 : a == 2 ? 7 : 9) + b - a;
}

// n floats in element order into LDS (4-byte loads: the sources are only 4-byte aligned)
__device__ __forceinline__ void stage(float *lds, const float *src, int n, int t)
{
    for (int i = t; i < n; i += THREADS) lds[i] = src[i];
}

__global__ void __launch_bounds__(THREADS) k_publish_othello(const OthelloPublishArgs a)
{
    __shared__ float buf[O_LDS];
    const int t = threadIdx.x;
    const int wg = blockIdx.x;
    int j = 0;
    while (j + 1 < a.n_jobs && wg >= a.first[j + 1]) ++j;
    const int part = wg - a.first[j];
    const OJob job = a.job[j];

    if (job.kind == O_EMBED) {
        const float *pos = job.src, *piece = job.aux, *legal = a.job[j + 1].src;
        for (int i = t; i < O_CELLS * 4 * (O_EMB / 8); i += THREADS) {
            const int row = i / (O_EMB / 8), c0 = 8 * (i % (O_EMB / 8));
            const int cell = row >> 2, kind = row & 3;
            const float *k = kind == 0 ? piece : kind == 1 ? piece + O_EMB : kind == 2 ? legal + O_EMB : legal;
            const float *p = pos + othello_orbit(cell) * O_EMB;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = p[c0 + e] + k[c0 + e];
            *reinterpret_cast<V8 *>(static_cast<uint16_t *>(job.dst) + row * O_EMB + c0) = pack8(v);
        }
    } else if (job.kind == O_CONV) {
        const int c_in = job.count & 0xffff, rows = (job.count >> 16) & 0xff, tiles = job.count >> 24;
        const int nkc = c_in / 32, tile = part / nkc, kc = part % nkc;
        for (int i = t; i < 16 * O_ROW; i += THREADS) {
            const int tl = i / O_ROW, r = i % O_ROW;
            buf[tl * O_ROW_PAD + r] = tl < rows ? job.src[(static_cast<int64_t>(16 * tile + tl) * c_in + 32 * kc) * TAPS + r] : 0.0f;
        }
        __syncthreads();
        for (int i = t; i < TAPS * 64; i += THREADS) {
            const int tap = i >> 6, lane = i & 63, g = lane >> 4, tl = lane & 15;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = buf[tl * O_ROW_PAD + (8 * g + e) * TAPS + tap];
            *reinterpret_cast<V8 *>(static_cast<uint16_t *>(job.dst) + ((static_cast<int64_t>(tap * nkc + kc) * tiles + tile) * 64 + lane) * 8) = pack8(v);
        }
    } else if (job.kind == O_BN) {
        const OJob second = a.job[j + 1];
        const int n = job.count & 0xffff, pad16 = job.count >> 16;
        float *scale = static_cast<float *>(job.dst), *shift = static_cast<float *>(second.dst);
        for (int i = t; i < n; i += THREADS) {
            const float s0 = job.aux[i] + a.bn_eps;
            const float root = sqrtf(s0);
            const float sc = job.src[i] / root;
            const float prod = second.aux[i] * sc;
            scale[i] = sc;
            shift[i] = second.src[i] - prod;
        }
        if (pad16 && t >= n && t < 16) { scale[t] = 1.0f; shift[t] = 0.0f; }
    } else if (job.kind == O_TRANS) {
        const int to = part / (O_FC / O_TILE), ti = part % (O_FC / O_TILE);         // the tile's first out row / in column, in tiles
        for (int i = t; i < O_TILE * O_TILE; i += THREADS) {
            const int r = i / O_TILE, c = i % O_TILE;
            buf[r * O_TILE_PAD + c] = job.src[(O_TILE * to + r) * O_FC + O_TILE * ti + c];
        }
        __syncthreads();
        float *dst = static_cast<float *>(job.dst);
        for (int i = t; i < O_TILE * O_TILE; i += THREADS) {
            const int r = i / O_TILE, c = i % O_TILE;                                // r: in, c: out
            dst[(O_TILE * ti + r) * O_FC + O_TILE * to + c] = buf[c * O_TILE_PAD + r];
        }
    } else if (job.kind == O_PERM16) {
        const int row0 = part * O_PERM_ROWS;
        stage(buf, job.src + row0 * O_FC, O_PERM_ROWS * O_FC, t);
        __syncthreads();
        for (int i = t; i < O_PERM_ROWS * O_CELLS; i += THREADS) {
            const int r = i / O_CELLS, cell = i % O_CELLS;
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = buf[r * O_FC + O_CELLS * c + cell];
            *reinterpret_cast<V8 *>(static_cast<uint16_t *>(job.dst) + (row0 + r) * O_FC + 8 * cell) = pack8(v);
        }
    } else if (job.kind == O_VCONV) {
        float *dst = static_cast<float *>(job.dst);
        for (int i = t; i < 8 * 72; i += THREADS) dst[i] = job.src[(i & 7) * 72 + (i >> 3)];
    } else if (job.kind == O_COPY) {
        float *dst = static_cast<float *>(job.dst);
        for (int i = t; i < job.count; i += THREADS) dst[i] = job.src[i];
    } else if (job.kind == O_BF16) {
        uint16_t *dst = static_cast<uint16_t *>(job.dst);
        for (int i = t; i < job.count; i += THREADS) dst[i] = bf16_bits(job.src[i]);
    } else if (job.kind == O_SCALARS) {
        float *dst = static_cast<float *>(job.dst);
        if (t == 0) dst[0] = *job.src;
        if (t == 1) dst[1] = *job.aux;
        if (t == 2) dst[2] = *a.job[j + 1].src;
    }
}

bool supported_conv(int c_in, int h_in, int pad)
{
    return (c_in == 32 && h_in == 8 && pad == 2) || (c_in == 256 && h_in == 10 && (pad == 1 || pad == 0)) || (c_in == 256 && h_in == 8 && pad == 1);
}

}  // namespace

extern "C" int az_nn_othello_publish_dev(const az_nn_othello_publish_src *src, const az_nn_othello_weights *dst, float *scalars_dev,
                                         void *stream)
{
    if (src == nullptr || dst == nullptr) return 1;
    if (src->n_body < 2 || src->n_body % 2 != 0 || src->n_convs != src->n_body + 2 || src->n_convs > AZ_NN_OTHELLO_MAX_CONVS) return 1;
    if (src->n_body != dst->n_body || src->n_convs != dst->n_convs) return 1;
    if (!(src->bn_eps >= 0.0f) || !(src->bn_eps <= 3.402823466e38f)) return 1;             // NaN, negative, infinite
    if (!aligned_to(scalars_dev, 4)) return 1;

    OthelloPublishArgs a{};
    int n = 0, wgs = 0;
    bool ok = true;
    auto w = [](const void *p) { return const_cast<void *>(p); };
    // an entry: a null destination only for the second entry of a job that needs three sources, an `aux` exactly for the
    // kinds that read one
    auto add = [&](const void *d, uintptr_t dst_align, const float *s, const float *aux, int32_t kind, int32_t count, int n_wg) {
        const bool reads_aux = kind == O_EMBED || kind == O_BN || kind == O_SCALARS || (kind == O_SECOND && d != nullptr);
        ok = ok && aligned_to(s, 4) && (reads_aux ? aligned_to(aux, 4) : aux == nullptr) &&
             (kind == O_SECOND && d == nullptr ? true : aligned_to(d, dst_align)) && n < O_MAX_JOBS;
        if (!ok) return;
        a.job[n] = OJob{w(d), s, aux, kind, count};
        a.first[n] = wgs;
        wgs += n_wg;
        ++n;
    };
    // a BatchNorm: 0 none, 1 complete, -1 only some of its four pointers
    auto have = [](const az_nn_othello_bn_src &b) {
        const int k = (b.weight != nullptr) + (b.bias != nullptr) + (b.mean != nullptr) + (b.var != nullptr);
        return k == 0 ? 0 : k == 4 ? 1 : -1;
    };
    auto bn = [&](const az_nn_othello_bn_src &b, const float *scale, const float *shift, int channels, int pad16) {
        ok = ok && have(b) == 1 && aligned_to(b.bias, 4) && aligned_to(b.mean, 4);
        if (!ok) return;
        add(scale, 4, b.weight, b.var, O_BN, channels | pad16 << 16, 1);
        add(shift, 4, b.bias, b.mean, O_SECOND, 0, 0);
    };
    auto copy = [&](const float *d, const float *s, int count) {
        if (d != nullptr && d == s) { ok = ok && aligned_to(s, 4); return; }           // an alias of the source: it already holds the value
        const uintptr_t x = reinterpret_cast<uintptr_t>(d), y = reinterpret_cast<uintptr_t>(s), bytes = 4u * static_cast<uintptr_t>(count);
        ok = ok && d != nullptr && s != nullptr && (x + bytes <= y || y + bytes <= x);
        add(d, 4, s, nullptr, O_COPY, count, 1);
    };
    const az_nn_othello_heads_weights &h = dst->heads;

    add(dst->embed_table, 16, src->pos_emb, src->piece_emb, O_EMBED, 0, 1);
    add(nullptr, 1, src->legal_emb, nullptr, O_SECOND, 0, 0);
    for (int i = 0; ok && i < src->n_convs; ++i) {
        const az_nn_othello_conv_layer &l = dst->conv[i];
        ok = ok && supported_conv(l.c_in, l.h_in, l.pad);
        if (!ok) break;
        add(l.w_packed, 16, src->conv_weight[i], nullptr, O_CONV, l.c_in | 16 << 16 | 16 << 24, 16 * (l.c_in / 32));
        const int pre = have(src->conv_pre[i]), post = have(src->conv_post[i]);
        ok = ok && pre >= 0 && post >= 0 && (l.pre_scale != nullptr) == (l.pre_shift != nullptr) && (l.pre_scale != nullptr) == (pre == 1);
        if (ok && pre == 1) bn(src->conv_pre[i], l.pre_scale, l.pre_shift, l.c_in, 0);
        if (ok && post == 1) bn(src->conv_post[i], l.post_scale, l.post_shift, O_CH, 0);
    }
    add(dst->dual_w16, 16, src->dual_weight, nullptr, O_CONV, O_CH | 8 << 16 | 1 << 24, O_CH / 32);
    bn(src->dual_bn, dst->dual_scale16, dst->dual_shift16, 8, 1);
    add(h.board_w, 2, src->board_weight, nullptr, O_BF16, O_CH, 1);
    copy(h.pass_norm_w, src->pass_norm_weight, O_CH);
    copy(h.pass_fc_w, src->pass_fc_weight, O_CH);
    add(h.v_conv_w, 4, src->v_conv_weight, nullptr, O_VCONV, 8 * 72, 1);
    bn(src->v_bn, h.v_bn_s, h.v_bn_b, 8, 0);
    copy(h.v_fc_w, src->v_fc_weight, 3 * 72);
    copy(h.v_fc_b, src->v_fc_bias, 3);
    add(h.a_fc_wt, 16, src->a_fc_weight, nullptr, O_TRANS, O_FC * O_FC, (O_FC / O_TILE) * (O_FC / O_TILE));
    if (h.a_fc_w16 != nullptr) add(h.a_fc_w16, 16, src->a_fc_weight, nullptr, O_PERM16, O_FC * O_FC, O_FC / O_PERM_ROWS);
    copy(h.a_fc_b, src->a_fc_bias, O_FC);
    copy(h.a_norm_w, src->a_norm_weight, O_FC);
    copy(h.a_out_w, src->a_out_weight, O_FC);
    add(scalars_dev, 4, src->board_bias, src->pass_fc_bias, O_SCALARS, 3, 1);
    add(nullptr, 1, src->a_out_bias, nullptr, O_SECOND, 0, 0);
    if (!ok) return 1;
    a.first[n] = wgs;
    a.n_jobs = n;
    a.bn_eps = src->bn_eps;
    hipLaunchKernelGGL(k_publish_othello, dim3(static_cast<unsigned>(wgs)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
