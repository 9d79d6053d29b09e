// train_stem_kernels.hip - the training forward and backward of the Connect4 stem (az_train_*stem* in az_train.h):
//   t[c][cell] = (state0[cell] * E[0][c] + state1[cell] * E[1][c]) + P[orbit(cell)][c];  y = silu(conv3x3(t, W) + b)
// kernels and host entry points in this one unit.  float32, 32 -> 64 channels, 6 x 7 cells, NCHW as torch holds it.
//
// The convolution is linear and t is a linear function of 26 "features" per cell: the two planes and the one-hot of the
// cell's orbit.  With Emb = [E; P] ([26][32]) and S[n][f][cell] those features, t = Emb^T S, and so
//   z[o][cell] = Pz[o][cell] + sum over taps inside the board, f < 2 of state_f[cell + tap] * T[o][f][tap]
//   T[o][f][tap] = sum_c W[o][c][tap] * E[f][c]           Pz = conv3x3(P[orbit(.)], W) + b
// (a K = 18 product per sample where the direct form has K = 288), and every parameter gradient follows from
//   G[o][f][tap] = sum over n, cell of dz[n][o][cell] * S[n][f][cell + tap]
// whose piece part (f < 2) is a 64 x 18 accumulator and whose position part needs only D[o][cell] = sum_n dz[n][o][cell],
// because the one-hot does not depend on n.  Five kernels:
//
//   k_stem_fold    the table (T [64][18], Pz [64][42]: 3840 floats, a function of the parameters alone) into the caller's
//                  workspace; workgroup o, one lane per entry, every 288-term sum down four interleaved chains.
//   k_stem_fwd     a workgroup of 192 lanes takes samples n = blockIdx, blockIdx + grid, ...  Lane 3 o + r owns output
//                  channel o on board rows 2 r and 2 r + 1: its 18 table weights and 14 Pz values stay in registers; per
//                  sample the two planes go into LDS as [2][8][9] with a ring of zeros (a tap outside the board reads a
//                  zero and a row cannot wrap), the lane reads its 2 x 4 x 9 window once, z goes through LDS to the
//                  lanes' own elements, silu, coalesced stores.
//   k_stem_bwd     the same mapping; a workgroup walks a contiguous run of samples.  Per sample z is formed again, dz =
//                  dy * silu'(z), D += dz (14 registers), G += dz * window (18 registers, this lane's rows only).  At the
//                  end the three lanes of a channel add their G in lane order and ONE partial row (D, G: 3840 floats)
//                  goes to the caller's workspace.
//   k_stem_reduce  one lane per element adds the rows in row order.
//   k_stem_unfold  workgroup o < 64: G[o][f][tap] for all 26 features (position part: D at the orbit's cells shifted by
//                  the tap), dW[o][c][tap] = sum_f G * Emb[f][c], db[o] = sum_cell D.  Workgroup 64 + f: dEmb[f][c] =
//                  sum over o, tap of G[o][f][tap] * W[o][c][tap] as eight chains of 72 added in order.
//
// No atomics, nothing cleared beforehand: two calls on the same inputs give the same bytes.  Sums are chains of fmaf.
// Plain C++ and vector stores only.
#include "engine_internal.h"

#include "az_train.h"
#include "train_common.h"

namespace az {
namespace {

constexpr int BLOCK = 192;                      // 64 channels x 3 row pairs
constexpr int CIN = 32, CH = 64, CELLS = ROWS * COLS, TAPS = 9;
constexpr int ACT = CH * CELLS;                 // 2688 values of a sample's output
constexpr int STATE = 3 * CELLS;                // 126 values of a sample's input; the third plane is not read
constexpr int OWN = ACT / BLOCK;                // 14 elements a lane owns: two board rows of one channel
constexpr int PIECE = 2 * TAPS;                 // 18: a channel's piece weights
constexpr int ORBITS = 24, FEATS = 2 + ORBITS;
constexpr int T_NUMEL = CH * PIECE;             // 1152
constexpr int TABLE_FLOATS = T_NUMEL + ACT;     // 3840: T, then Pz
constexpr int ROW_FLOATS = ACT + T_NUMEL;       // 3840: D, then G's piece part
constexpr int W_NUMEL = CH * CIN * TAPS;        // 18432
constexpr int FWD_GRID = 1024;
constexpr int UNFOLD_BLOCK = 256;
static_assert(OWN * BLOCK == ACT && OWN == 2 * COLS && BLOCK == 3 * CH, "a lane owns two board rows of one channel");
static_assert(TABLE_FLOATS * 4 == AZ_TRAIN_STEM_TABLE_BYTES && ROW_FLOATS % 4 == 0, "the table's size is part of the ABI");
static_assert(T_NUMEL % BLOCK == 0, "the piece part of a row is written in whole rounds");

struct StemArgs {
    const float *state, *E, *P, *W, *b, *dy, *table;
    float *y, *table_out;
    float *dE, *dP, *dW, *db, *sum, *ws;        // sum: the added row; ws: the partial rows
    int64_t N, per;                             // per: the run of samples a backward workgroup walks
    int rows;                                   // backward workgroups = partial rows
};

__device__ __forceinline__ int orbit(int cell) { const int c = cell % COLS; return 4 * (cell / COLS) + (c < COLS - 1 - c ? c : COLS - 1 - c); }

__global__ void __launch_bounds__(64) k_stem_fold(StemArgs a)
{
    __shared__ float w[CIN * TAPS];             // this channel's filter, [c][tap]
    __shared__ float emb[FEATS * CIN];
    const int o = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < CIN * TAPS; i += 64) w[i] = a.W[o * CIN * TAPS + i];
    for (int i = tid; i < FEATS * CIN; i += 64) emb[i] = i < 2 * CIN ? a.E[i] : a.P[i - 2 * CIN];
    __syncthreads();
    if (tid < CELLS) {
        // Pz[o][cell]: taps in tap order, channels down four interleaved chains, a tap outside the board skipped
        const int row = tid / COLS, col = tid % COLS;
        float part[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int t = 0; t < TAPS; ++t) {
            const int r = row + t / 3 - 1, c = col + t % 3 - 1;
            if (r < 0 || r >= ROWS || c < 0 || c >= COLS) continue;
            const float *p = emb + (2 + orbit(r * COLS + c)) * CIN;
            for (int ch = 0; ch < CIN; ch += 4)
#pragma unroll
                for (int u = 0; u < 4; ++u) part[u] = fmaf(w[(ch + u) * TAPS + t], p[ch + u], part[u]);
        }
        a.table_out[T_NUMEL + o * CELLS + tid] = ((part[0] + part[1]) + (part[2] + part[3])) + a.b[o];
    } else if (tid < CELLS + PIECE) {
        const int i = tid - CELLS, f = i / TAPS, t = i % TAPS;
        float part[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int ch = 0; ch < CIN; ch += 4)
#pragma unroll
            for (int u = 0; u < 4; ++u) part[u] = fmaf(w[(ch + u) * TAPS + t], emb[f * CIN + ch + u], part[u]);
        a.table_out[o * PIECE + i] = (part[0] + part[1]) + (part[2] + part[3]);
    }
}

// what a lane keeps over all of its samples: its channel's piece weights and its 14 cells' Pz
struct Lane {
    float T[PIECE], pz[OWN];
};

__device__ __forceinline__ void load_lane(const float *__restrict__ table, Lane &l)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < PIECE; ++i) l.T[i] = table[(tid / 3) * PIECE + i];
#pragma unroll
    for (int i = 0; i < OWN; ++i) l.pz[i] = table[T_NUMEL + tid * OWN + i];
}

// the sample's two planes into the ringed image; the ring stays zero
__device__ __forceinline__ void stage_planes(const float *__restrict__ state, float *sp)
{
    const int tid = threadIdx.x;
    if (tid < 2 * CELLS) sp[(tid / CELLS) * PAD + ring_pos(tid % CELLS)] = state[tid];
}

// the lane's window: ring rows 2 r .. 2 r + 3 (board rows 2 r - 1 .. 2 r + 2), all nine ring columns, both planes
__device__ __forceinline__ void load_window(const float *sp, float s[2][4][PW])
{
    const int r = threadIdx.x % 3;
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int y = 0; y < 4; ++y)
#pragma unroll
            for (int x = 0; x < PW; ++x) s[f][y][x] = sp[f * PAD + (2 * r + y) * PW + x];
}

// z of the lane's 14 cells: Pz, then the 18 piece terms in (plane, tap) order
__device__ __forceinline__ void lane_z(const Lane &l, const float s[2][4][PW], float z[OWN])
{
#pragma unroll
    for (int i = 0; i < OWN; ++i) {
        const int lr = i / COLS, col = i % COLS;
        float v = l.pz[i];
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int t = 0; t < TAPS; ++t) v = fmaf(s[f][lr + t / 3][col + t % 3], l.T[f * TAPS + t], v);
        z[i] = v;
    }
}

__global__ void __launch_bounds__(BLOCK) k_stem_fwd(StemArgs a)
{
    __shared__ float sp[2 * PAD];
    __shared__ float zb[ACT];
    const int tid = threadIdx.x;
    Lane l;
    load_lane(a.table, l);
    if (tid < 2 * PAD) sp[tid] = 0.0f;
    __syncthreads();                            // the clearing touches the boards too: it ends before any sample is stored
    for (int64_t n = blockIdx.x; n < a.N; n += gridDim.x) {
        stage_planes(a.state + n * STATE, sp);
        __syncthreads();
        float s[2][4][PW], z[OWN];
        load_window(sp, s);
        lane_z(l, s, z);
#pragma unroll
        for (int i = 0; i < OWN; ++i) zb[tid * OWN + i] = z[i];
        __syncthreads();                        // every window is read: the next sample's planes may go in after this
        float *ys = a.y + n * ACT;
#pragma unroll
        for (int j = 0; j < OWN; ++j) {
            const float v = zb[tid + j * BLOCK];
            ys[tid + j * BLOCK] = v * sigmoid(v);
        }
        // zb is written again only after the next sample's first barrier, which every lane reaches after these reads
    }
}

__global__ void __launch_bounds__(BLOCK) k_stem_bwd(StemArgs a)
{
    __shared__ float sp[2 * PAD];
    __shared__ float gp[BLOCK * PIECE];
    const int tid = threadIdx.x;
    Lane l;
    load_lane(a.table, l);
    if (tid < 2 * PAD) sp[tid] = 0.0f;
    __syncthreads();                            // the clearing touches the boards too: it ends before any sample is stored

    float D[OWN], G[PIECE];
#pragma unroll
    for (int i = 0; i < OWN; ++i) D[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < PIECE; ++i) G[i] = 0.0f;

    const int64_t n0 = static_cast<int64_t>(blockIdx.x) * a.per;
    const int64_t n1 = n0 + a.per < a.N ? n0 + a.per : a.N;
    for (int64_t n = n0; n < n1; ++n) {
        stage_planes(a.state + n * STATE, sp);
        const float2 *dys = reinterpret_cast<const float2 *>(a.dy + n * ACT + tid * OWN);    // 56 bytes a lane, 8-byte aligned
        float dz[OWN];
#pragma unroll
        for (int i = 0; i < OWN / 2; ++i) {
            const float2 v = dys[i];
            dz[2 * i] = v.x;
            dz[2 * i + 1] = v.y;
        }
        __syncthreads();
        float s[2][4][PW], z[OWN];
        load_window(sp, s);
        __syncthreads();                        // every window is read: the next sample's planes may go in after this
        lane_z(l, s, z);
#pragma unroll
        for (int i = 0; i < OWN; ++i) {
            dz[i] = dz[i] * dsilu(z[i]);
            D[i] += dz[i];
        }
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int t = 0; t < TAPS; ++t) {
                float g = G[f * TAPS + t];
#pragma unroll
                for (int i = 0; i < OWN; ++i) g = fmaf(dz[i], s[f][i / COLS + t / 3][i % COLS + t % 3], g);
                G[f * TAPS + t] = g;
            }
    }

    float *row = a.ws + static_cast<size_t>(blockIdx.x) * ROW_FLOATS;
#pragma unroll
    for (int i = 0; i < OWN; ++i) row[tid * OWN + i] = D[i];
#pragma unroll
    for (int i = 0; i < PIECE; ++i) gp[tid * PIECE + i] = G[i];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < T_NUMEL / BLOCK; ++j) {
        const int e = tid + j * BLOCK, o = e / PIECE, i = e % PIECE;
        row[ACT + e] = (gp[(3 * o) * PIECE + i] + gp[(3 * o + 1) * PIECE + i]) + gp[(3 * o + 2) * PIECE + i];
    }
}

__global__ void __launch_bounds__(UNFOLD_BLOCK) k_stem_reduce(StemArgs a)
{
    const int i = blockIdx.x * UNFOLD_BLOCK + threadIdx.x;
    if (i >= ROW_FLOATS) return;
    float v = 0.0f;
    for (int r = 0; r < a.rows; ++r) v += a.ws[static_cast<size_t>(r) * ROW_FLOATS + i];
    a.sum[i] = v;
}

// G[o][2 + k][tap] from D: the cells of orbit k (one in the middle column, else two in column order), each shifted back
// by the tap; a source outside the board contributes nothing
__device__ __forceinline__ float position_g(const float *__restrict__ D_o, int k, int tap)
{
    const int row = k / 4, c0 = k % 4;
    const int sr = row - (tap / 3 - 1);
    if (sr < 0 || sr >= ROWS) return 0.0f;
    float v = 0.0f;
    const int a0 = c0 - (tap % 3 - 1), a1 = COLS - 1 - c0 - (tap % 3 - 1);
    if (a0 >= 0 && a0 < COLS) v += D_o[sr * COLS + a0];
    if (c0 != COLS - 1 - c0 && a1 >= 0 && a1 < COLS) v += D_o[sr * COLS + a1];
    return v;
}

__global__ void __launch_bounds__(UNFOLD_BLOCK) k_stem_unfold(StemArgs a)
{
    __shared__ float g[CH * TAPS];              // 576: workgroup o uses [26][9], workgroup 64 + f uses [64][9]
    __shared__ float parts[8 * CIN];
    const int tid = threadIdx.x;
    const float *D = a.sum, *Gp = a.sum + ACT;
    if (blockIdx.x < CH) {
        const int o = blockIdx.x;
        if (tid < FEATS * TAPS) {
            const int f = tid / TAPS, t = tid % TAPS;
            g[tid] = f < 2 ? Gp[o * PIECE + tid] : position_g(D + o * CELLS, f - 2, t);
        }
        __syncthreads();
        for (int e = tid; e < CIN * TAPS; e += UNFOLD_BLOCK) {
            const int c = e / TAPS, t = e % TAPS;
            float v = 0.0f;
            for (int f = 0; f < FEATS; ++f) v = fmaf(g[f * TAPS + t], f < 2 ? a.E[f * CIN + c] : a.P[(f - 2) * CIN + c], v);
            a.dW[o * CIN * TAPS + e] = v;
        }
        if (tid == UNFOLD_BLOCK - 1) {
            float v = 0.0f;
            for (int cell = 0; cell < CELLS; ++cell) v += D[o * CELLS + cell];
            a.db[o] = v;
        }
    } else {
        const int f = blockIdx.x - CH;
        for (int e = tid; e < CH * TAPS; e += UNFOLD_BLOCK) {
            const int o = e / TAPS, t = e % TAPS;
            g[e] = f < 2 ? Gp[o * PIECE + f * TAPS + t] : position_g(D + o * CELLS, f - 2, t);
        }
        __syncthreads();
        const int c = tid % CIN, part = tid / CIN;          // eight chains of eight output channels each
        float v = 0.0f;
        for (int o = 8 * part; o < 8 * part + 8; ++o)
#pragma unroll
            for (int t = 0; t < TAPS; ++t) v = fmaf(g[o * TAPS + t], a.W[(o * CIN + c) * TAPS + t], v);
        parts[part * CIN + c] = v;
        __syncthreads();
        if (tid < CIN) {
            float s = parts[tid];
            for (int p = 1; p < 8; ++p) s += parts[p * CIN + tid];
            if (f < 2) a.dE[f * CIN + tid] = s;
            else a.dP[(f - 2) * CIN + tid] = s;
        }
    }
}

// the workspace: the forward's table, the added row, the partial rows
int64_t workspace_bytes(int rows) { return AZ_TRAIN_STEM_TABLE_BYTES + rows_bytes(1 + rows, ROW_FLOATS); }

}  // namespace
}  // namespace az

using namespace az::host;

namespace {

void stem_inputs(const std::string &w, const az_train_stem_params *p, const float *state, int64_t N, az::StemArgs &a)
{
    require(n_ok(N), w + ": N must be positive (and at most 2^30)");
    require(p != nullptr, w + ": null argument");
    require(aligned(state, 4) && aligned(p->piece_emb, 4) && aligned(p->pos_emb, 4) && aligned(p->conv_weight, 4) &&
            aligned(p->conv_bias, 4), w + ": state, piece_emb, pos_emb, conv_weight or conv_bias null or misaligned");
    a.state = state; a.N = N;
    a.E = p->piece_emb; a.P = p->pos_emb; a.W = p->conv_weight; a.b = p->conv_bias;
}

}  // namespace

extern "C" {

int64_t az_train_stem_workspace_bytes(int64_t N, int max_workgroups)
{
    if (!n_ok(N) || max_workgroups < 0) return -1;
    return az::workspace_bytes(partition(N, max_workgroups).rows);
}

int az_train_dev_stem_fwd(const az_train_stem_params *params, const float *state, int64_t N, float *y,
                          void *workspace, int64_t workspace_bytes, void *stream)
{
    return guarded([&] {
        const std::string w("az_train_dev_stem_fwd");
        az::StemArgs a{};
        stem_inputs(w, params, state, N, a);
        require(aligned(y, 16), w + ": a null y or one that is not 16-byte aligned");
        require(aligned(workspace, 16), w + ": a null workspace or one that is not 16-byte aligned");
        require(workspace_bytes >= AZ_TRAIN_STEM_TABLE_BYTES, w + ": a workspace smaller than AZ_TRAIN_STEM_TABLE_BYTES");
        a.y = y; a.table_out = static_cast<float *>(workspace); a.table = a.table_out;
        const hipStream_t s = static_cast<hipStream_t>(stream);
        hipLaunchKernelGGL(az::k_stem_fold, dim3(az::CH), dim3(64), 0, s, a);
        hipLaunchKernelGGL(az::k_stem_fwd, dim3(fwd_grid(N, az::FWD_GRID)), dim3(az::BLOCK), 0, s, a);
        HIP_OK(hipGetLastError());
    });
}

int az_train_dev_stem_bwd(const az_train_stem_params *params, const float *state, const float *table, const float *dy,
                          int64_t N, int max_workgroups, const az_train_stem_grads *grads, void *stream)
{
    return guarded([&] {
        const std::string w("az_train_dev_stem_bwd");
        az::StemArgs a{};
        stem_inputs(w, params, state, N, a);
        require(max_workgroups >= 0, w + ": max_workgroups must not be negative");
        require(grads != nullptr, w + ": null argument");
        require(aligned(table, 16) && aligned(dy, 16) && aligned(grads->workspace, 16),
                w + ": table, dy or workspace null or not 16-byte aligned");
        require(aligned(grads->d_piece_emb, 4) && aligned(grads->d_pos_emb, 4) && aligned(grads->d_conv_weight, 4) &&
                aligned(grads->d_conv_bias, 4), w + ": d_piece_emb, d_pos_emb, d_conv_weight or d_conv_bias null or misaligned");
        const Runs runs = partition(N, max_workgroups);
        a.per = runs.per; a.rows = runs.rows;
        require(grads->workspace_bytes >= az::workspace_bytes(a.rows), w + ": a workspace smaller than az_train_stem_workspace_bytes says");
        a.table = table; a.dy = dy;
        a.dE = grads->d_piece_emb; a.dP = grads->d_pos_emb; a.dW = grads->d_conv_weight; a.db = grads->d_conv_bias;
        a.sum = static_cast<float *>(grads->workspace) + az::TABLE_FLOATS;      // the table's place is left alone
        a.ws = a.sum + az::ROW_FLOATS;
        const hipStream_t s = static_cast<hipStream_t>(stream);
        hipLaunchKernelGGL(az::k_stem_bwd, dim3(a.rows), dim3(az::BLOCK), 0, s, a);
        hipLaunchKernelGGL(az::k_stem_reduce, dim3((az::ROW_FLOATS + az::UNFOLD_BLOCK - 1) / az::UNFOLD_BLOCK), dim3(az::UNFOLD_BLOCK), 0, s, a);
        hipLaunchKernelGGL(az::k_stem_unfold, dim3(az::CH + az::FEATS), dim3(az::UNFOLD_BLOCK), 0, s, a);
        HIP_OK(hipGetLastError());
    });
}

}  // extern "C"
