// optim_kernels.hip - the learner's optimiser side: the gradient norm over every parameter, its clipping and the AdamW
// step (az_opt_* in az_train.h), kernels and host entry points in this one unit.  What the reference does after
// `backward()` with `clip_grad_norm_` and `torch.optim.AdamW.step()` - a norm per tensor, a stack, a norm, a clamp, a
// multiply and about a dozen `_foreach_*` passes - is three launches for up to SLICE tensors:
//
//   k_opt_sqsum       one workgroup per (tensor, chunk of CHUNK elements), looked up in a chunk table built at create
//                     time.  16-byte loads where the gradient's address allows, one element per lane otherwise and for a
//                     tail; the lanes' sums go through wave_sum (nn_common.h), the four wavefronts' through LDS, added in
//                     a fixed order; ONE partial per chunk in the handle's workspace.
//   k_opt_norm        one workgroup adds the partials in a fixed order (lane l takes l, l + 256, ...; wave_sum; the four
//                     wavefronts), writes total_norm = sqrt(sum) and coef = min(1, max_norm / (total_norm + 1e-6)).
//   k_opt_clip_adamw  the same mapping as k_opt_sqsum; per element, float32, in the order az_train.h states.
//
// The gradients' addresses change every step (autograd allocates afresh after zero_grad(set_to_none=True)): they travel
// as KERNEL ARGUMENTS, SLICE tensors to a launch, next to the two scalars that depend on a tensor's own step number and
// the per-group scalars - no staging buffer, no copy, no wait, no allocation.  More than SLICE tensors loop the first
// and the third launch over slices.  Parameter and moment addresses sit in a device table written by az_opt_bind.
// No atomics: two calls on the same inputs give the same bytes.  Gradients are read, never written.  Plain C++ and
// vector stores only.
#include "engine_internal.h"

#include "az_train.h"
#include "nn_common.h"

namespace az {
namespace {

constexpr int WAVE = 64;
constexpr int BLOCK = 256, WAVES = BLOCK / WAVE;
constexpr int VEC = 4;                  // floats of a 16-byte access
constexpr int CHUNK = 2048;             // elements a workgroup owns: two 16-byte accesses per lane
constexpr int SLICE = 96;               // tensors whose gradient addresses one launch carries
static_assert(CHUNK % (BLOCK * VEC) == 0, "a chunk is whole rounds of the workgroup's vector stride");

struct TensorRec {                      // device table, one per tensor; p, m, v from az_opt_bind
    float *p, *m, *v;
    int64_t numel;
    int32_t group, pad;
};
struct ChunkRec { int32_t tensor, chunk; };      // the chunk's elements start at chunk * CHUNK of its tensor
struct GroupHp { float decay, one_m_beta1, beta2, one_m_beta2, eps; };

struct SliceArgs {
    const TensorRec *tensors;
    const ChunkRec *chunks;
    float *partials;                    // [chunks of all slices]
    const float *coef;                  // what k_opt_norm left; null: no clipping
    int32_t first_tensor, first_chunk;  // of this slice
    const float *grad[SLICE];           // null: the tensor is skipped whole
    float step_size[SLICE], inv_sqrt_bc2[SLICE];
    GroupHp hp[AZ_OPT_MAX_GROUPS];
};
static_assert(sizeof(SliceArgs) <= 2048, "a slice stays well under the 4 KB of kernel arguments");

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ bool vec_ok(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the workgroup's chunk: its tensor (as an index into the slice too), where it starts and how many elements it has
struct Chunk { int t, local; int64_t start; int n; };
__device__ __forceinline__ Chunk my_chunk(const SliceArgs &a)
{
    const ChunkRec cr = a.chunks[a.first_chunk + static_cast<int>(blockIdx.x)];
    Chunk c;
    c.t = uniform(cr.tensor);
    c.local = c.t - a.first_tensor;
    c.start = static_cast<int64_t>(uniform(cr.chunk)) * CHUNK;
    const int64_t left = a.tensors[c.t].numel - c.start;
    c.n = left < CHUNK ? static_cast<int>(left) : CHUNK;
    return c;
}

// the four wavefronts' sums, added in a fixed order; the result is valid in thread 0
__device__ __forceinline__ float block_sum(float v, float *lds)
{
    v = wave_sum(v);
    if (threadIdx.x % WAVE == 0) lds[threadIdx.x / WAVE] = v;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__global__ void __launch_bounds__(BLOCK) k_opt_sqsum(SliceArgs a)
{
    __shared__ float lds[WAVES];
    const Chunk c = my_chunk(a);
    const float *g = a.grad[c.local];
    const int tid = threadIdx.x;
    float acc = 0.0f;
    if (g != nullptr) {
        g += c.start;
        if (vec_ok(g)) {
            const int nv = c.n & ~(VEC - 1);
            for (int i = tid * VEC; i < nv; i += BLOCK * VEC) {
                const float4 x = *reinterpret_cast<const float4 *>(g + i);
                acc += x.x * x.x; acc += x.y * x.y; acc += x.z * x.z; acc += x.w * x.w;
            }
            if (nv + tid < c.n) acc += g[nv + tid] * g[nv + tid];
        } else {
            for (int i = tid; i < c.n; i += BLOCK) acc += g[i] * g[i];
        }
    }
    const float total = block_sum(acc, lds);
    if (tid == 0) a.partials[a.first_chunk + blockIdx.x] = total;
}

__global__ void __launch_bounds__(BLOCK) k_opt_norm(const float *partials, int n, float max_norm, float *grad_norm, float *coef)
{
    __shared__ float lds[WAVES];
    float acc = 0.0f;
    for (int i = threadIdx.x; i < n; i += BLOCK) acc += partials[i];
    const float sum = block_sum(acc, lds);
    if (threadIdx.x != 0) return;
    const float total = sqrtf(sum);
    const float c = max_norm / (total + 1e-6f);
    *grad_norm = total;
    *coef = c > 1.0f ? 1.0f : c;        // a NaN stays one, as torch.clamp(max=1) leaves it
}

struct Update {
    bool clip;
    float coef, decay, one_m_beta1, beta2, one_m_beta2, eps, step_size, inv_sqrt_bc2;
};

// one element; both the vector and the scalar path go through here, so a tensor's result does not depend on its address
__device__ __forceinline__ void update(const Update &u, float g, float &p, float &m, float &v)
{
    if (u.clip) g = g * u.coef;
    p = p * u.decay;
    m = m + (g - m) * u.one_m_beta1;
    v = v * u.beta2 + (u.one_m_beta2 * g) * g;
    p = p - u.step_size * (m / (sqrtf(v) * u.inv_sqrt_bc2 + u.eps));
}

// one element through memory: every value is read before any is written
__device__ __forceinline__ void update_at(const Update &u, const float *g, float *p, float *m, float *v, int i)
{
    const float gg = g[i];
    float pp = p[i], mm = m[i], vv = v[i];
    update(u, gg, pp, mm, vv);
    p[i] = pp; m[i] = mm; v[i] = vv;
}

__global__ void __launch_bounds__(BLOCK) k_opt_clip_adamw(SliceArgs a)
{
    const Chunk c = my_chunk(a);
    const float *g = a.grad[c.local];
    if (g == nullptr) return;
    const TensorRec r = a.tensors[c.t];
    const GroupHp h = a.hp[uniform(r.group)];
    Update u;
    u.clip = a.coef != nullptr;
    u.coef = u.clip ? *a.coef : 1.0f;
    u.decay = h.decay; u.one_m_beta1 = h.one_m_beta1; u.beta2 = h.beta2; u.one_m_beta2 = h.one_m_beta2; u.eps = h.eps;
    u.step_size = a.step_size[c.local];
    u.inv_sqrt_bc2 = a.inv_sqrt_bc2[c.local];
    g += c.start;
    float *p = r.p + c.start, *m = r.m + c.start, *v = r.v + c.start;
    const int tid = threadIdx.x;
    if (vec_ok(g) && vec_ok(p) && vec_ok(m) && vec_ok(v)) {
        const int nv = c.n & ~(VEC - 1);
        for (int i = tid * VEC; i < nv; i += BLOCK * VEC) {
            const float4 gg = *reinterpret_cast<const float4 *>(g + i);
            float4 pp = *reinterpret_cast<const float4 *>(p + i);
            float4 mm = *reinterpret_cast<const float4 *>(m + i);
            float4 vv = *reinterpret_cast<const float4 *>(v + i);
            update(u, gg.x, pp.x, mm.x, vv.x);
            update(u, gg.y, pp.y, mm.y, vv.y);
            update(u, gg.z, pp.z, mm.z, vv.z);
            update(u, gg.w, pp.w, mm.w, vv.w);
            *reinterpret_cast<float4 *>(p + i) = pp;
            *reinterpret_cast<float4 *>(m + i) = mm;
            *reinterpret_cast<float4 *>(v + i) = vv;
        }
        const int i = nv + tid;
        if (i < c.n) update_at(u, g, p, m, v, i);
    } else {
        for (int i = tid; i < c.n; i += BLOCK) update_at(u, g, p, m, v, i);
    }
}

}  // namespace
}  // namespace az

struct az_opt {
    int64_t n = 0;
    int32_t n_groups = 0;
    std::vector<az::TensorRec> rec;             // host copy of the device table
    std::vector<az::ChunkRec> chunks;
    std::vector<int32_t> first_chunk;           // per slice, and the total behind the last
    std::vector<az::SliceArgs> slices;          // filled anew by every step: no allocation there
    bool bound = false;
    DevBuf<az::TensorRec> d_rec;
    DevBuf<az::ChunkRec> d_chunks;
    DevBuf<float> d_work;                       // one partial per chunk, then the clip coefficient
    int64_t n_slices() const { return static_cast<int64_t>(slices.size()); }
    int64_t n_chunks() const { return static_cast<int64_t>(chunks.size()); }
};

extern "C" {

int az_opt_create(int64_t n_tensors, const int64_t *numel, const int32_t *group, int32_t n_groups, az_opt **out)
{
    return guarded([&] {
        const std::string w("az_opt_create");
        require(out != nullptr && numel != nullptr && group != nullptr, w + ": null argument");
        *out = nullptr;
        require(n_tensors > 0 && n_tensors <= (int64_t(1) << 20), w + ": n_tensors must be positive (and at most 2^20)");
        require(n_groups >= 1 && n_groups <= AZ_OPT_MAX_GROUPS, w + ": n_groups must lie in [1, 16]");
        int64_t total = 0;
        for (int64_t i = 0; i < n_tensors; ++i) {
            require(numel[i] > 0 && numel[i] <= (int64_t(1) << 40), w + ": numel must be positive (and at most 2^40)");
            require(group[i] >= 0 && group[i] < n_groups, w + ": a group index outside [0, n_groups)");
            total += (numel[i] + az::CHUNK - 1) / az::CHUNK;
        }
        require(total <= (int64_t(1) << 30), w + ": more than 2^30 chunks");
        auto o = std::make_unique<az_opt>();
        o->n = n_tensors;
        o->n_groups = n_groups;
        o->rec.resize(static_cast<size_t>(n_tensors));
        o->chunks.reserve(static_cast<size_t>(total));
        for (int64_t i = 0; i < n_tensors; ++i) {
            if (i % az::SLICE == 0) o->first_chunk.push_back(static_cast<int32_t>(o->chunks.size()));
            o->rec[i] = az::TensorRec{nullptr, nullptr, nullptr, numel[i], group[i], 0};
            const int64_t k = (numel[i] + az::CHUNK - 1) / az::CHUNK;
            for (int64_t c = 0; c < k; ++c) o->chunks.push_back(az::ChunkRec{static_cast<int32_t>(i), static_cast<int32_t>(c)});
        }
        o->first_chunk.push_back(static_cast<int32_t>(o->chunks.size()));
        o->slices.resize(o->first_chunk.size() - 1);
        *out = o.release();
    });
}

void az_opt_destroy(az_opt *o) { delete o; }

int az_opt_bind(az_opt *o, void *const *param, void *const *exp_avg, void *const *exp_avg_sq)
{
    return guarded([&] {
        const std::string w("az_opt_bind");
        require(o != nullptr && param != nullptr && exp_avg != nullptr && exp_avg_sq != nullptr, w + ": null argument");
        for (int64_t i = 0; i < o->n; ++i)
            require(aligned(param[i], 4) && aligned(exp_avg[i], 4) && aligned(exp_avg_sq[i], 4),
                    w + ": a null address or one that is not 4-byte aligned");
        for (int64_t i = 0; i < o->n; ++i) {
            o->rec[i].p = static_cast<float *>(param[i]);
            o->rec[i].m = static_cast<float *>(exp_avg[i]);
            o->rec[i].v = static_cast<float *>(exp_avg_sq[i]);
        }
        o->bound = false;
        HIP_OK(hipDeviceSynchronize());         // an earlier step may still be reading the table
        o->d_rec.ensure(o->rec.size());
        o->d_chunks.ensure(o->chunks.size());
        o->d_work.ensure(o->chunks.size() + 1);
        HIP_OK(hipMemcpy(o->d_rec.p, o->rec.data(), o->rec.size() * sizeof(az::TensorRec), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(o->d_chunks.p, o->chunks.data(), o->chunks.size() * sizeof(az::ChunkRec), hipMemcpyHostToDevice));
        o->bound = true;
    });
}

int az_opt_dev_step(az_opt *o, const void *const *grad, const int64_t *step, const double *group_hp, float max_norm,
                    float *grad_norm, void *stream)
{
    return guarded([&] {
        const std::string w("az_opt_dev_step");
        require(o != nullptr && grad != nullptr && step != nullptr && group_hp != nullptr, w + ": null argument");
        require(o->bound, w + ": called before az_opt_bind");
        require(!std::isnan(max_norm), w + ": max_norm is not a number");
        const bool clip = max_norm > 0.0f;
        if (clip) require(aligned(grad_norm, 4), w + ": a null or misaligned grad_norm");
        az::GroupHp hp[AZ_OPT_MAX_GROUPS] = {};
        for (int g = 0; g < o->n_groups; ++g) {
            const double *h = group_hp + g * AZ_OPT_GROUP_HP;
            const double lr = h[0], b1 = h[1], b2 = h[2], eps = h[3], wd = h[4];
            require(lr >= 0.0 && std::isfinite(lr), w + ": lr must not be negative");
            require(b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0, w + ": a beta outside [0, 1)");
            require(eps >= 0.0 && std::isfinite(eps), w + ": eps must not be negative");
            require(wd >= 0.0 && std::isfinite(wd), w + ": weight_decay must not be negative");
            hp[g] = az::GroupHp{static_cast<float>(1.0 - lr * wd), static_cast<float>(1.0 - b1), static_cast<float>(b2),
                                static_cast<float>(1.0 - b2), static_cast<float>(eps)};
        }
        for (int64_t i = 0; i < o->n; ++i) {
            require(step[i] >= 0, w + ": a negative step");
            require(step[i] == 0 || grad[i] != nullptr, w + ": a positive step with a null gradient");
            require(grad[i] == nullptr || (step[i] > 0 && aligned(grad[i], 4)),
                    w + ": a gradient with step 0 or one that is not 4-byte aligned");
        }
        // the two scalars of a tensor's own step number, in double, rounded once; tensors of a group mostly share it
        int64_t seen_t[AZ_OPT_MAX_GROUPS];
        float seen_size[AZ_OPT_MAX_GROUPS], seen_bc2[AZ_OPT_MAX_GROUPS];
        for (auto &t : seen_t) t = 0;
        float *work = o->d_work.p, *coef = work + o->n_chunks();
        for (int64_t s = 0; s < o->n_slices(); ++s) {
            az::SliceArgs &a = o->slices[s];
            a.tensors = o->d_rec.p; a.chunks = o->d_chunks.p; a.partials = work; a.coef = clip ? coef : nullptr;
            a.first_tensor = static_cast<int32_t>(s * az::SLICE);
            a.first_chunk = o->first_chunk[s];
            std::memcpy(a.hp, hp, sizeof(hp));
            for (int j = 0; j < az::SLICE; ++j) {
                const int64_t i = s * az::SLICE + j;
                const bool on = i < o->n && grad[i] != nullptr;
                a.grad[j] = on ? static_cast<const float *>(grad[i]) : nullptr;
                a.step_size[j] = a.inv_sqrt_bc2[j] = 0.0f;
                if (!on) continue;
                const int g = o->rec[i].group;
                if (seen_t[g] != step[i]) {
                    const double *h = group_hp + g * AZ_OPT_GROUP_HP;
                    const double t = static_cast<double>(step[i]);
                    seen_t[g] = step[i];
                    seen_size[g] = static_cast<float>(h[0] / (1.0 - std::pow(h[1], t)));
                    seen_bc2[g] = static_cast<float>(1.0 / std::sqrt(1.0 - std::pow(h[2], t)));
                }
                a.step_size[j] = seen_size[g];
                a.inv_sqrt_bc2[j] = seen_bc2[g];
            }
        }
        const hipStream_t st = static_cast<hipStream_t>(stream);
        auto blocks = [&](int64_t s) { return dim3(static_cast<unsigned>(o->first_chunk[s + 1] - o->first_chunk[s])); };
        if (clip) {
            for (int64_t s = 0; s < o->n_slices(); ++s)
                hipLaunchKernelGGL(az::k_opt_sqsum, blocks(s), dim3(az::BLOCK), 0, st, o->slices[s]);
            hipLaunchKernelGGL(az::k_opt_norm, dim3(1), dim3(az::BLOCK), 0, st, work, static_cast<int>(o->n_chunks()), max_norm,
                               grad_norm, coef);
        }
        for (int64_t s = 0; s < o->n_slices(); ++s)
            hipLaunchKernelGGL(az::k_opt_clip_adamw, blocks(s), dim3(az::BLOCK), 0, st, o->slices[s]);
        HIP_OK(hipGetLastError());
    });
}

}  // extern "C"
