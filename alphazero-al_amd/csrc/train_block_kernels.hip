// train_block_kernels.hip - the learner's first network piece: the training forward and backward of the Connect4
// residual block  y = x + keep * silu(conv3x3(GroupNorm1(x)))  (az_train_*block* in az_train.h), kernels and host entry
// points in this one unit.  float32, 64 channels, 6 x 7 cells, NCHW as torch holds it.  Three kernels:
//
//   k_block_fwd     a workgroup of four wavefronts takes samples n = blockIdx, blockIdx + grid, ...  Per sample: the
//                   2688 values into registers (11 per lane), mean and variance as two block sums, the normalised
//                   sample into LDS as [64][8][9] with a ring of zeros round every channel's board (so a tap outside
//                   the board reads a zero and a row cannot wrap), z = W * xn as a 64 x 48 x 576 product on
//                   v_mfma_f32_16x16x4_f32 (wavefront w owns output channels 16w .. 16w + 15 and three tiles of 16
//                   cells; cells 42 .. 47 are computed on cell 0's data and dropped), z through LDS back to the
//                   lanes' own elements, bias, silu, keep, the skip connection, coalesced stores.
//   k_block_bwd     a workgroup walks a contiguous run of samples.  Per sample: xn and dz into two ringed LDS images;
//                   dW += dz * xn-windows as a 64 x 576 x 44 product (wavefront w owns input channels 16w .. 16w + 15,
//                   that is 4 x 9 tiles: 144 accumulator registers a lane, the whole 64 x 576 gradient across the
//                   workgroup, kept over all of its samples); dxn = conv_transpose(dz, W) as the forward's product
//                   with the taps mirrored and W read as [c][o]; db, dbeta, dgamma as sums of four lanes per channel,
//                   kept in a register over the samples; dx from two more block sums.  At the end ONE partial row
//                   (dW, db, dgamma, dbeta: 37056 floats) in the caller's workspace.
//   k_block_reduce  one lane per parameter-gradient element adds the rows in row order.
//
// In both products the lane's quarter of an MFMA's K (lane / 16) is a channel (4 * step + quarter) and the tap is
// uniform, so every LDS and W offset of the unrolled nine taps is an immediate; W comes straight from global memory
// (144 KB, L2-resident), the next channel group's nine values are loaded while this group's 27 MFMAs run.  The 576
// terms of an output go down four interleaved accumulation chains that are added at the end.
// An MFMA here is a k-ordered chain of float32 fused multiply-adds: exact float32, nothing narrower anywhere.
// No atomics, nothing cleared beforehand: two calls on the same inputs give the same bytes.  Plain C++ and vector
// stores only.
#include "engine_internal.h"

#include "az_train.h"
#include "nn_common.h"
#include "train_common.h"

namespace az {
namespace {

constexpr int WAVE = 64;
constexpr int BLOCK = 256, WAVES = BLOCK / WAVE;
constexpr int CH = 64, CELLS = ROWS * COLS, TAPS = 9;
constexpr int ACT = CH * CELLS;                 // 2688 values of a sample
constexpr int KK = CH * TAPS;                   // 576: a filter's weights
constexpr int PER_LANE = (ACT + BLOCK - 1) / BLOCK;      // 11 elements a lane owns (the last round is half full)
constexpr int CELL_TILES = 3;                   // 48 cells in tiles of 16
constexpr int CELL_STEPS = 11;                  // 44 cells in K steps of 4
constexpr int SPLIT = 4;                        // independent accumulation chains of the 576-term products
constexpr int W_NUMEL = CH * KK;                // 36864
constexpr int ROW_FLOATS = W_NUMEL + 3 * CH;    // a partial row: dW, db, dgamma, dbeta
constexpr int FWD_GRID = 2048;
static_assert(ROW_FLOATS % 4 == 0, "rows of the workspace stay 16-byte aligned");
static_assert(SPLIT == 4 && (CH / 4) % SPLIT == 0, "the chains are added as (0 + 1) + (2 + 3)");
static_assert(CELL_TILES * 16 >= CELLS && CELL_STEPS * 4 >= CELLS && CH % 16 == 0 && 16 * TAPS == 9 * 16, "tile shapes");

struct BlockArgs {
    const float *x, *gamma, *beta, *W, *b, *keep, *dy;
    const float *z_in, *stats_in;
    float *y, *z_out, *stats_out;
    float *dx, *dgamma, *dbeta, *dW, *db, *ws;
    int64_t N, per;                             // per: the run of samples a backward workgroup walks
    int rows;                                   // backward workgroups = partial rows
    float eps;
};

// two block sums at once, each the four wavefronts' sums in a fixed order; every lane gets both.  Local to this file:
// the attention kernel's only sum across wavefronts (its d_q_norm, d_k_norm tail) adds 16-lane columns it staged itself,
// not nn_common.h's wave_sum of a whole wavefront, so the two do not mean the same additions.
__device__ __forceinline__ void block_sum2(float &a, float &b, float *red)
{
    a = wave_sum(a);
    b = wave_sum(b);
    const int w = threadIdx.x / WAVE;
    if (threadIdx.x % WAVE == 0) { red[w] = a; red[WAVES + w] = b; }
    __syncthreads();
    a = ((red[0] + red[1]) + red[2]) + red[3];
    b = ((red[4] + red[5]) + red[6]) + red[7];
    __syncthreads();
}

// one block sum, the same order
__device__ __forceinline__ float block_sum(float a, float *red)
{
    a = wave_sum(a);
    if (threadIdx.x % WAVE == 0) red[threadIdx.x / WAVE] = a;
    __syncthreads();
    a = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return a;
}

// The 64 x 48 x 576 product both passes share.  src: a ringed LDS image [64][PAD].  Forward (FLIP false):
// acc[row o][cell] = sum over c, tap of W[o][c][tap] * src[c][cell's window at tap].  Backward (FLIP true):
// acc[row c][cell] = sum over o, tap of W[o][c][tap] * src[o][cell's window at the mirrored tap].
// acc[j][r] is row 16 * wave + 4 * (lane / 16) + r, cell 16 * j + lane % 16.
template <bool FLIP>
__device__ __forceinline__ void conv_mfma(const float *__restrict__ Wg, const float *src, f4 acc[CELL_TILES])
{
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    const int row = wave * 16 + (lane & 15), kq = lane >> 4;
    const float *a_ptr = Wg + (FLIP ? kq * KK + row * TAPS : row * KK + kq * TAPS);
    constexpr int A_STEP = FLIP ? 4 * KK : 4 * TAPS;
    int corner[CELL_TILES];                     // the window's first tap in this lane's channel of a group of four
    f4 part[SPLIT][CELL_TILES];                 // four interleaved chains of 144 terms each, not one of 576: less rounding
#pragma unroll
    for (int j = 0; j < CELL_TILES; ++j) {
        const int cell = j * 16 + (lane & 15);
        const int cc = cell < CELLS ? cell : 0;
        corner[j] = kq * PAD + (cc / COLS) * PW + cc % COLS;
#pragma unroll
        for (int u = 0; u < SPLIT; ++u) part[u][j] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    float a_next[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; ++t) a_next[t] = a_ptr[t];
    for (int g0 = 0; g0 < CH / 4; g0 += SPLIT) {
#pragma unroll
        for (int u = 0; u < SPLIT; ++u) {
            const int g = g0 + u;
            float a[TAPS];
#pragma unroll
            for (int t = 0; t < TAPS; ++t) a[t] = a_next[t];
            const float *nxt = a_ptr + (g + 1 < CH / 4 ? g + 1 : g) * A_STEP;
#pragma unroll
            for (int t = 0; t < TAPS; ++t) a_next[t] = nxt[t];
            const float *s = src + g * 4 * PAD;
#pragma unroll
            for (int t = 0; t < TAPS; ++t) {
                const int ky = t / 3, kx = t % 3;
                const int off = FLIP ? (2 - ky) * PW + (2 - kx) : ky * PW + kx;
#pragma unroll
                for (int j = 0; j < CELL_TILES; ++j)
                    part[u][j] = mfma(a[t], s[corner[j] + off], part[u][j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < CELL_TILES; ++j) acc[j] = (part[0][j] + part[1][j]) + (part[2][j] + part[3][j]);
}

// the product's result to an LDS image [64][42]
__device__ __forceinline__ void store_tiles(const f4 acc[CELL_TILES], float *dst)
{
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
#pragma unroll
    for (int j = 0; j < CELL_TILES; ++j) {
        const int cell = j * 16 + (lane & 15);
        if (cell >= CELLS) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[(wave * 16 + 4 * (lane >> 4) + r) * CELLS + cell] = acc[j][r];
    }
}

__global__ void __launch_bounds__(BLOCK) k_block_fwd(BlockArgs a)
{
    __shared__ float xnp[CH * PAD];
    __shared__ float zb[ACT];
    __shared__ float red[WAVES];
    const int tid = threadIdx.x;
    for (int i = tid; i < CH * PAD; i += BLOCK) xnp[i] = 0.0f;          // the rings stay zero from here on
    __syncthreads();                            // the clearing touches the boards too: it ends before any sample is stored
    for (int64_t n = blockIdx.x; n < a.N; n += gridDim.x) {
        const float *xs = a.x + n * ACT;
        float xv[PER_LANE];
        float sum = 0.0f;
#pragma unroll
        for (int j = 0; j < PER_LANE; ++j) {
            const int e = tid + j * BLOCK;
            xv[j] = e < ACT ? xs[e] : 0.0f;
            sum += xv[j];
        }
        const float mean = block_sum(sum, red) / static_cast<float>(ACT);
        float sq = 0.0f;
#pragma unroll
        for (int j = 0; j < PER_LANE; ++j) {
            const float d = tid + j * BLOCK < ACT ? xv[j] - mean : 0.0f;
            sq += d * d;
        }
        const float rstd = 1.0f / sqrtf(block_sum(sq, red) / static_cast<float>(ACT) + a.eps);
#pragma unroll
        for (int j = 0; j < PER_LANE; ++j) {
            const int e = tid + j * BLOCK;
            if (e >= ACT) continue;
            const int c = e / CELLS;
            xnp[c * PAD + ring_pos(e % CELLS)] = (xv[j] - mean) * rstd * a.gamma[c] + a.beta[c];
        }
        __syncthreads();
        f4 acc[CELL_TILES];
        conv_mfma<false>(a.W, xnp, acc);
        store_tiles(acc, zb);
        __syncthreads();
        float *ys = a.y + n * ACT;
#pragma unroll
        for (int j = 0; j < PER_LANE; ++j) {
            const int e = tid + j * BLOCK;
            if (e >= ACT) continue;
            const int c = e / CELLS;
            const float z = zb[e] + a.b[c];
            const float k = a.keep != nullptr ? a.keep[n * CH + c] : 1.0f;
            ys[e] = xv[j] + k * (z * sigmoid(z));
            if (a.z_out != nullptr) a.z_out[n * ACT + e] = z;
        }
        if (a.stats_out != nullptr && tid == 0) {
            a.stats_out[2 * n] = mean;
            a.stats_out[2 * n + 1] = rstd;
        }
    }
}

// a channel's sum over its 42 cells of an LDS image [64][stride] (at `pos(cell)`): lane 4c + q adds cells q, q + 4,
// ..., then the four lanes of a channel add up; all four hold the total
template <class Pos>
__device__ __forceinline__ float channel_sum(const float *img, int stride, Pos pos)
{
    const int c = threadIdx.x >> 2, q = threadIdx.x & 3;
    float v = 0.0f;
    for (int cell = q; cell < CELLS; cell += 4) v += img[c * stride + pos(cell)];
    v += __shfl_xor(v, 1, WAVE);
    v += __shfl_xor(v, 2, WAVE);
    return v;
}

__global__ void __launch_bounds__(BLOCK) k_block_bwd(BlockArgs a)
{
    __shared__ float xnp[CH * PAD];
    __shared__ float dzp[CH * PAD];
    __shared__ float gb[ACT];                   // dxn, lanes' own elements
    __shared__ float hb[ACT];                   // dxn * xhat
    __shared__ float red[2 * WAVES];
    const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE, kq = lane >> 4;
    for (int i = tid; i < CH * PAD; i += BLOCK) { xnp[i] = 0.0f; dzp[i] = 0.0f; }
    __syncthreads();                            // the clearing touches the boards too: it ends before any sample is stored

    f4 dw[4][TAPS];                             // tile (16 output channels mt) x (16 of this wavefront's 144 (c, tap))
    int noff[TAPS];                             // this lane's (c, tap) of tile j as an offset into xnp
#pragma unroll
    for (int j = 0; j < TAPS; ++j) {
        const int kk = j * 16 + (lane & 15), tap = kk % TAPS;
        noff[j] = (wave * 16 + kk / TAPS) * PAD + (tap / 3) * PW + tap % 3;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) dw[mt][j] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    float p_db = 0.0f, p_dgamma = 0.0f, p_dbeta = 0.0f;          // channel tid / 4, the same in its four lanes

    const int64_t n0 = static_cast<int64_t>(blockIdx.x) * a.per;
    const int64_t n1 = n0 + a.per < a.N ? n0 + a.per : a.N;
    for (int64_t n = n0; n < n1; ++n) {
        const float *xs = a.x + n * ACT, *zs = a.z_in + n * ACT, *dys = a.dy + n * ACT;
        const float mean = a.stats_in[2 * n], rstd = a.stats_in[2 * n + 1];
        float xhat[PER_LANE], dyv[PER_LANE];
#pragma unroll
        for (int j = 0; j < PER_LANE; ++j) {
            const int e = tid + j * BLOCK;
            xhat[j] = dyv[j] = 0.0f;
            if (e >= ACT) continue;
            const int c = e / CELLS, at = c * PAD + ring_pos(e % CELLS);
            xhat[j] = (xs[e] - mean) * rstd;
            dyv[j] = dys[e];
            xnp[at] = xhat[j] * a.gamma[c] + a.beta[c];
            const float z = zs[e], s = sigmoid(z);
            const float k = a.keep != nullptr ? a.keep[n * CH + c] : 1.0f;
            dzp[at] = dyv[j] * k * (s + z * s * (1.0f - s));        // dsilu(z) spelled out: the call gives this kernel other registers
        }
        __syncthreads();
        p_db += channel_sum(dzp, PAD, [](int cell) { return ring_pos(cell); });

        // dW: K runs over the cells, four to a step; cells 42 and 43 read a zero of dz's ring
#pragma unroll 1
        for (int s = 0; s < CELL_STEPS; ++s) {
            const int cell = 4 * s + kq;
            const bool on = cell < CELLS;
            const int a_pos = on ? ring_pos(cell) : 0;
            const int b_pos = on ? (cell / COLS) * PW + cell % COLS : 0;
            float av[4], bv[TAPS];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) av[mt] = dzp[(mt * 16 + (lane & 15)) * PAD + a_pos];
#pragma unroll
            for (int j = 0; j < TAPS; ++j) bv[j] = xnp[noff[j] + b_pos];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int j = 0; j < TAPS; ++j)
                    dw[mt][j] = mfma(av[mt], bv[j], dw[mt][j]);
        }

        f4 acc[CELL_TILES];
        conv_mfma<true>(a.W, dzp, acc);
        store_tiles(acc, gb);
        __syncthreads();
        float m1 = 0.0f, m2 = 0.0f;
        float g[PER_LANE];
#pragma unroll
        for (int j = 0; j < PER_LANE; ++j) {
            const int e = tid + j * BLOCK;
            g[j] = 0.0f;
            if (e >= ACT) continue;
            const float dxn = gb[e];
            hb[e] = dxn * xhat[j];
            g[j] = dxn * a.gamma[e / CELLS];
            m1 += g[j];
            m2 += g[j] * xhat[j];
        }
        block_sum2(m1, m2, red);                // hb is whole after its first barrier
        m1 = m1 / static_cast<float>(ACT);
        m2 = m2 / static_cast<float>(ACT);
        p_dbeta += channel_sum(gb, CELLS, [](int cell) { return cell; });
        p_dgamma += channel_sum(hb, CELLS, [](int cell) { return cell; });
        float *dxs = a.dx + n * ACT;
#pragma unroll
        for (int j = 0; j < PER_LANE; ++j) {
            const int e = tid + j * BLOCK;
            if (e < ACT) dxs[e] = dyv[j] + rstd * (g[j] - m1 - xhat[j] * m2);
        }
        __syncthreads();                        // gb and hb are read to the end before the next sample's images go in
    }

    float *row = a.ws + static_cast<size_t>(blockIdx.x) * ROW_FLOATS;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int j = 0; j < TAPS; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                row[(mt * 16 + 4 * kq + r) * KK + wave * 16 * TAPS + j * 16 + (lane & 15)] = dw[mt][j][r];
    if ((tid & 3) == 0) {
        const int c = tid >> 2;
        row[W_NUMEL + c] = p_db;
        row[W_NUMEL + CH + c] = p_dgamma;
        row[W_NUMEL + 2 * CH + c] = p_dbeta;
    }
}

__global__ void __launch_bounds__(BLOCK) k_block_reduce(BlockArgs a)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= ROW_FLOATS) return;
    float v = 0.0f;
    for (int r = 0; r < a.rows; ++r) v += a.ws[static_cast<size_t>(r) * ROW_FLOATS + i];
    if (i < W_NUMEL) a.dW[i] = v;
    else if (i < W_NUMEL + CH) a.db[i - W_NUMEL] = v;
    else if (i < W_NUMEL + 2 * CH) a.dgamma[i - W_NUMEL - CH] = v;
    else a.dbeta[i - W_NUMEL - 2 * CH] = v;
}

}  // namespace
}  // namespace az

using namespace az::host;

namespace {

void block_inputs(const std::string &w, const az_train_block_params *p, const float *x, const float *keep, int64_t N,
                  az::BlockArgs &a)
{
    require(n_ok(N), w + ": N must be positive (and at most 2^30)");
    require(p != nullptr, w + ": null argument");
    require(aligned(x, 16) && aligned(p->conv_weight, 16), w + ": x or conv_weight null or not 16-byte aligned");
    require(keep == nullptr || aligned(keep, 16), w + ": a keep that is not 16-byte aligned");
    require(aligned(p->norm_weight, 4) && aligned(p->norm_bias, 4) && aligned(p->conv_bias, 4),
            w + ": norm_weight, norm_bias or conv_bias null or misaligned");
    a.x = x; a.keep = keep; a.N = N;
    a.gamma = p->norm_weight; a.beta = p->norm_bias; a.W = p->conv_weight; a.b = p->conv_bias;
}

}  // namespace

extern "C" {

int64_t az_train_block_workspace_bytes(int64_t N, int max_workgroups)
{
    if (!n_ok(N) || max_workgroups < 0) return -1;
    return rows_bytes(partition(N, max_workgroups).rows, az::ROW_FLOATS);
}

int az_train_dev_block_fwd(const az_train_block_params *params, const float *x, const float *keep, int64_t N, float eps,
                           float *y, const az_train_block_saved *saved, void *stream)
{
    return guarded([&] {
        const std::string w("az_train_dev_block_fwd");
        az::BlockArgs a{};
        block_inputs(w, params, x, keep, N, a);
        require(eps > 0.0f && std::isfinite(eps), w + ": eps must be positive");
        require(aligned(y, 16), w + ": a null y or one that is not 16-byte aligned");
        if (saved != nullptr && (saved->z != nullptr || saved->stats != nullptr)) {
            require(aligned(saved->z, 16), w + ": a null saved z or one that is not 16-byte aligned");
            require(aligned(saved->stats, 4), w + ": a null or misaligned saved stats");
            a.z_out = saved->z; a.stats_out = saved->stats;
        }
        a.y = y; a.eps = eps;
        hipLaunchKernelGGL(az::k_block_fwd, dim3(fwd_grid(N, az::FWD_GRID)), dim3(az::BLOCK), 0, static_cast<hipStream_t>(stream), a);
        HIP_OK(hipGetLastError());
    });
}

int az_train_dev_block_bwd(const az_train_block_params *params, const float *x, const float *keep, const float *dy,
                           const az_train_block_saved *saved, int64_t N, int max_workgroups,
                           const az_train_block_grads *grads, void *stream)
{
    return guarded([&] {
        const std::string w("az_train_dev_block_bwd");
        az::BlockArgs a{};
        block_inputs(w, params, x, keep, N, a);
        require(max_workgroups >= 0, w + ": max_workgroups must not be negative");
        require(saved != nullptr && grads != nullptr, w + ": null argument");
        require(aligned(dy, 16) && aligned(saved->z, 16) && aligned(grads->dx, 16) && aligned(grads->d_conv_weight, 16) &&
                aligned(grads->workspace, 16), w + ": dy, saved z, dx, d_conv_weight or workspace null or not 16-byte aligned");
        require(aligned(saved->stats, 4) && aligned(grads->d_norm_weight, 4) && aligned(grads->d_norm_bias, 4) &&
                aligned(grads->d_conv_bias, 4), w + ": saved stats, d_norm_weight, d_norm_bias or d_conv_bias null or misaligned");
        const Runs runs = partition(N, max_workgroups);
        a.per = runs.per; a.rows = runs.rows;
        require(grads->workspace_bytes >= rows_bytes(a.rows, az::ROW_FLOATS),
                w + ": a workspace smaller than az_train_block_workspace_bytes says");
        a.dy = dy; a.z_in = saved->z; a.stats_in = saved->stats;
        a.dx = grads->dx; a.dgamma = grads->d_norm_weight; a.dbeta = grads->d_norm_bias; a.dW = grads->d_conv_weight;
        a.db = grads->d_conv_bias; a.ws = static_cast<float *>(grads->workspace);
        const hipStream_t s = static_cast<hipStream_t>(stream);
        hipLaunchKernelGGL(az::k_block_bwd, dim3(a.rows), dim3(az::BLOCK), 0, s, a);
        hipLaunchKernelGGL(az::k_block_reduce, dim3((az::ROW_FLOATS + az::BLOCK - 1) / az::BLOCK), dim3(az::BLOCK), 0, s, a);
        HIP_OK(hipGetLastError());
    });
}

}  // extern "C"
