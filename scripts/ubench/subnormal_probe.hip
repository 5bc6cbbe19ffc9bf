// Probe: do the f64 / f32 operations the numeric kernels accumulate with keep subnormal operands and results on gfx950?
// The hash / dense classes add into LDS with ds_add_f64 (atomicAdd on a __shared__ double), the register classes with
// VALU adds; fp32 products are v_mul_f32.  One wave, one case per lane, the operands as kernel arguments (nothing folds
// at compile time); the host compares every result bit for bit with the IEEE one.  Built with the library's flags:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 subnormal_probe.hip -o subnormal_probe && ./subnormal_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

constexpr int kCases = 6;

struct In {
    double d[kCases][2];   // f64 operand pairs
    float f[kCases][2];    // f32 operand pairs
};
struct Out {
    double lds_add[kCases], glb_add[kCases], valu_add[kCases], valu_mul[kCases];
    float lds_add_f32[kCases], valu_mul_f32[kCases], valu_add_f32[kCases];
};

__global__ __launch_bounds__(64) void probe(In in, Out* out)
{
    __shared__ double sd[64];
    __shared__ float sf[64];
    const int i = threadIdx.x;
    if (i < kCases) {
        sd[i] = in.d[i][0];
        sf[i] = in.f[i][0];
    }
    __syncthreads();
    if (i < kCases) {
        atomicAdd(&sd[i], in.d[i][1]);                   // ds_add_f64
        atomicAdd(&sf[i], in.f[i][1]);                   // ds_add_f32
        out->glb_add[i] = in.d[i][0];
    }
    __syncthreads();
    if (i < kCases) {
        atomicAdd(&out->glb_add[i], in.d[i][1]);         // global f64 atomic add
        out->lds_add[i] = sd[i];
        out->lds_add_f32[i] = sf[i];
        out->valu_add[i] = in.d[i][0] + in.d[i][1];
        out->valu_mul[i] = in.d[i][0] * in.d[i][1];
        out->valu_mul_f32[i] = in.f[i][0] * in.f[i][1];
        out->valu_add_f32[i] = in.f[i][0] + in.f[i][1];
    }
}

#define CHECK(x)                                                                              \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) {                                                               \
            std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__);        \
            return 2;                                                                         \
        }                                                                                     \
    } while (0)

template <typename T>
static int report(const char* what, const T* got, const T* want)
{
    int bad = 0;
    for (int c = 0; c < kCases; ++c) {
        const bool same = std::memcmp(&got[c], &want[c], sizeof(T)) == 0;
        bad += !same;
        std::printf("%-16s case %d: got %-24a want %-24a %s\n", what, c, (double)got[c], (double)want[c],
                    same ? "kept" : "DIFFERS");
    }
    return bad;
}

int main()
{
    const double s = std::ldexp(1.0, -1074), n = std::ldexp(1.0, -1022);
    const float sf = std::ldexp(1.0f, -149), nf = std::ldexp(1.0f, -126);
    In in{};
    // f64: 0 + sub, sub + sub, normal - normal -> sub, sub + normal, a product below the normal range, 0 + max sub
    const double d[kCases][2] = {{0.0, 3 * s}, {5 * s, 7 * s}, {n, -(n - 9 * s)}, {11 * s, n}, {std::ldexp(3.0, -530), std::ldexp(5.0, -530)},
                                 {0.0, n - s}};
    const float f[kCases][2] = {{0.0f, 3 * sf}, {5 * sf, 7 * sf}, {nf, -(nf - 9 * sf)}, {11 * sf, nf},
                                {std::ldexp(3.0f, -70), std::ldexp(5.0f, -70)}, {0.0f, nf - sf}};
    std::memcpy(in.d, d, sizeof d);
    std::memcpy(in.f, f, sizeof f);
    Out want{};
    for (int c = 0; c < kCases; ++c) {
        want.lds_add[c] = want.glb_add[c] = want.valu_add[c] = d[c][0] + d[c][1];
        want.valu_mul[c] = d[c][0] * d[c][1];
        want.lds_add_f32[c] = want.valu_add_f32[c] = f[c][0] + f[c][1];
        want.valu_mul_f32[c] = f[c][0] * f[c][1];
    }
    Out* d_out = nullptr;
    CHECK(hipMalloc(&d_out, sizeof(Out)));
    CHECK(hipMemset(d_out, 0, sizeof(Out)));
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, in, d_out);
    CHECK(hipGetLastError());
    Out got{};
    CHECK(hipMemcpy(&got, d_out, sizeof(Out), hipMemcpyDeviceToHost));
    CHECK(hipFree(d_out));
    int bad = 0;
    bad += report("ds_add_f64", got.lds_add, want.lds_add);
    bad += report("global_add_f64", got.glb_add, want.glb_add);
    bad += report("v_add_f64", got.valu_add, want.valu_add);
    bad += report("v_mul_f64", got.valu_mul, want.valu_mul);
    bad += report("ds_add_f32", got.lds_add_f32, want.lds_add_f32);
    bad += report("v_add_f32", got.valu_add_f32, want.valu_add_f32);
    bad += report("v_mul_f32", got.valu_mul_f32, want.valu_mul_f32);
    std::printf("%s: %d of %d results differ from IEEE (subnormals %s)\n", bad ? "FLUSH" : "OK", bad, 7 * kCases,
                bad ? "flushed somewhere" : "kept everywhere");
    return 0;
}
