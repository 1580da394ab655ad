// Additions to hip/hip_runtime.h for the fp32 MFMA kernels of the coordinate MLP (csrc/atlas.hip, csrc/atlas_bwd.hip): what
// those two files use beyond the simple kernels, mapped to host code with the hardware's data layout.  A header of its own,
// so that the checks built on hip_gemm.h compile as before.
//   * v_mfma_f32_32x32x2_f32: a wave collective; lane l supplies A[l % 32][l / 32] and B[l / 32][l % 32], and register r of
//     lane l holds D[8 (r / 4) + 4 (l / 32) + r % 4][l % 32].  Each product is fused into the running sum (k = 0, then 1).
//   * `extern __shared__ smem[]` becomes a block-scope redeclaration of `cpuhip_smem`, which the check defines with
//     CPUHIP_DEFINE_LDS in the namespace that encloses the kernel (define CPUHIP_DYNAMIC_LDS_ONLY before hip/hip_runtime.h).
//   * float2, readfirstlane, hipMemsetAsync and the launcher's attribute call.
#pragma once
#include <string.h>

#define smem cpuhip_smem
#define CPUHIP_DEFINE_LDS alignas(16) unsigned char cpuhip_smem[160 * 1024];

struct float2 { float x, y; };
#define __builtin_amdgcn_readfirstlane(x) (x)

constexpr int hipFuncAttributeMaxDynamicSharedMemorySize = 0;
static inline hipError_t hipFuncSetAttribute(const void*, int, int) { return hipSuccess; }
static inline hipError_t hipMemsetAsync(void* p, int value, size_t bytes, hipStream_t) {
    memset(p, value, bytes);
    return hipSuccess;
}

typedef float cpuhip_f32x16 __attribute__((ext_vector_type(16)));
static inline cpuhip_f32x16 cpuhip_mfma_32x32x2_f32(float a, float b, cpuhip_f32x16 c, int, int, int) {
    struct Slot { float a, b; };
    Slot* s = static_cast<Slot*>(cpuhip::ctx.wave_scratch);
    const int l = (int)(cpuhip::ctx.tid.x & 63);
    s[l].a = a;
    s[l].b = b;
    cpuhip::ctx.wave_bar->arrive_and_wait();
    const int col = l & 31, hi = l >> 5;
    cpuhip_f32x16 d = c;
    for (int r = 0; r < 16; ++r) {
        const int row = 8 * (r >> 2) + 4 * hi + (r & 3);
        d[r] = fmaf(s[row + 32].a, s[col + 32].b, fmaf(s[row].a, s[col].b, d[r]));
    }
    cpuhip::ctx.wave_bar->arrive_and_wait();
    return d;
}
#define __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, x, y, z) cpuhip_mfma_32x32x2_f32(a, b, c, x, y, z)
