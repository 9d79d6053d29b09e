// nn_selftest.hip - debug entry points that run one helper of nn_common.h on caller-supplied lanes, so that a test can
// pin the helper itself and not only the kernels built from it.  Nothing on the evaluator's path calls these.
#include "az_nn.h"
#include "nn_common.h"

namespace {

// one wavefront: lane l reduces a[l] and b[l] over the four rows of its column, paired and one at a time
__global__ void __launch_bounds__(64) k_col_reduce2(const float *a, const float *b, float *out)
{
    const int lane = threadIdx.x;
    const float va = a[lane], vb = b[lane];
    float sa = va, sb = vb, ma = va, mb = vb;
    col_sum2(sa, sb);
    col_max2(ma, mb);
    out[0 * 64 + lane] = sa;
    out[1 * 64 + lane] = sb;
    out[2 * 64 + lane] = col_sum(va);
    out[3 * 64 + lane] = col_sum(vb);
    out[4 * 64 + lane] = ma;
    out[5 * 64 + lane] = mb;
    out[6 * 64 + lane] = col_max(va);
    out[7 * 64 + lane] = col_max(vb);
}

}  // namespace

extern "C" int az_nn_debug_col_reduce2(const float *a, const float *b, float *out, void *stream)
{
    if (a == nullptr || b == nullptr || out == nullptr) return 1;
    hipLaunchKernelGGL(k_col_reduce2, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a, b, out);
    return 0;
}
