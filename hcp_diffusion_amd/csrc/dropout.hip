// dropout.hip — LoRA layer-output dropout (reference lora_base_patch.py:74) with a counter-based mask that is never stored.
//
// The mask is a pure function of (seed, forward count, layer, element index): Philox4x32-10 with
//   counter = (lo32(group_base + g), hi32(group_base + g), layer_id, lo32(calls)),  key = (lo32(seed), hi32(seed))
// where g is the index of a group of 8 consecutive bf16 elements (one 16-byte access) and (seed, calls) are read from a device
// int64[2] state tensor — nothing that varies per step is a kernel argument, so one captured graph serves every step.  The four
// output words are eight 16-bit lanes: element 8g + 2j takes the low half of word j, element 8g + 2j + 1 the high half.  An element
// is kept iff its lane is >= T = round(p * 65536); survivors are scaled by 1 / (1 - T / 65536), the EFFECTIVE probability
// (p = 0.1: T = 6554, 0.100006).  32-bit lanes would need two Philox calls per 16-byte access; the integer VALU work is what this
// kernel pays for.  The backward regenerates the same mask from the same state: dx = keep ? dy * scale : 0.
// `calls` enters with its low 32 bits: the stream of a (seed, layer) repeats after 2^32 forwards.
// Grid-stride over groups, 16-byte loads and stores, no atomics, no workspace; out may alias y (each thread reads its own 16 bytes
// before it writes them).
#include "hcp_common.h"
#include "hcp_philox.h"             // philox4x32_10: shared with sampler.hip

namespace {

constexpr int DROP_THREADS = 256;
constexpr long DROP_MAX_BLOCKS = 2048;          // kernels.DROPOUT_MAX_THREADS = DROP_MAX_BLOCKS * DROP_THREADS
inline int drop_grid(long groups) {
    long g = (groups + DROP_THREADS - 1) / DROP_THREADS;
    if (g > DROP_MAX_BLOCKS) g = DROP_MAX_BLOCKS;
    if (g < 1) g = 1;
    return (int)g;
}

// out = bf16(keep ? y * scale : 0 (+ res)); res == null: the backward form (y = dy, out = dx)
HCP_KERNEL(256) dropout_kernel(const hcp_bf16* y, const hcp_bf16* res, hcp_bf16* out, long groups, const long long* state,
                               uint32_t layer_id, unsigned long long group_base, uint32_t T, float scale) {
    const unsigned long long seed = (unsigned long long)state[0];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), calls = (uint32_t)(unsigned long long)state[1];
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
        const unsigned long long ctr = group_base + (unsigned long long)g;
        uint32_t w[4];
        philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), layer_id, calls, k0, k1, w);
        const hcp_bf16x8 v = *(const hcp_bf16x8*)(y + g * 8);
        const hcp_bf16x8 r = res ? *(const hcp_bf16x8*)(res + g * 8) : hcp_zero8();
        hcp_bf16x8 o;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const uint32_t lane = (q & 1) ? (w[q >> 1] >> 16) : (w[q >> 1] & 0xffffu);
            float f = lane >= T ? hcp_bf2f((unsigned short)v[q]) * scale : 0.0f;
            if (res) f += hcp_bf2f((unsigned short)r[q]);
            o[q] = (short)hcp_f2bf(f);
        }
        *(hcp_bf16x8*)(out + g * 8) = o;
    }
}

HCP_KERNEL(64) dropout_advance_kernel(long long* state) {
    if (threadIdx.x == 0) state[1] += 1;
}

inline bool drop_threshold(double p, uint32_t* T, float* scale) {
    if (!(p >= 0.0)) return false;                     // negative or NaN
    const double t = p >= 1.0 ? 65536.0 : nearbyint(p * 65536.0);
    *T = (uint32_t)t;
    *scale = *T >= 65536u ? 0.0f : 1.0f / (1.0f - (float)*T / 65536.0f);
    return true;
}

}  // namespace

// out[n] = bf16(keep ? y * scale : 0 (+ residual)), fp32 arithmetic, one rounding; residual may be NULL, out may alias y.
// state: device int64[2] = (seed, calls).  n % 8 == 0, 16-byte aligned contiguous buffers.
HCP_API int hcp_dropout_residual_fwd(const void* y, const void* residual, void* out, long n, const long long* state, unsigned layer_id,
                                     unsigned long long group_base, double p, hipStream_t stream) {
    uint32_t T; float scale;
    HCP_REQUIRE(y && out && state && n > 0 && n % 8 == 0, "hcp_dropout_residual_fwd: n must be a positive multiple of 8");
    HCP_REQUIRE((((size_t)y | (size_t)residual | (size_t)out) & 15) == 0, "hcp_dropout_residual_fwd: buffers must be 16-byte aligned");
    HCP_REQUIRE(drop_threshold(p, &T, &scale), "hcp_dropout_residual_fwd: p must be >= 0");
    HCP_LAUNCH(dropout_kernel, dim3(drop_grid(n / 8)), dim3(DROP_THREADS), 0, stream, (const hcp_bf16*)y, (const hcp_bf16*)residual,
               (hcp_bf16*)out, n / 8, state, (uint32_t)layer_id, group_base, T, scale);
    HCP_LAUNCH_CHECK("dropout_residual_fwd");
}

// dx[n] = keep ? dy * scale : 0 with the mask of the forward that ran on the same (state, layer_id, group_base, p); dx may alias dy.
HCP_API int hcp_dropout_bwd(const void* dy, void* dx, long n, const long long* state, unsigned layer_id, unsigned long long group_base,
                            double p, hipStream_t stream) {
    uint32_t T; float scale;
    HCP_REQUIRE(dy && dx && state && n > 0 && n % 8 == 0, "hcp_dropout_bwd: n must be a positive multiple of 8");
    HCP_REQUIRE((((size_t)dy | (size_t)dx) & 15) == 0, "hcp_dropout_bwd: buffers must be 16-byte aligned");
    HCP_REQUIRE(drop_threshold(p, &T, &scale), "hcp_dropout_bwd: p must be >= 0");
    HCP_LAUNCH(dropout_kernel, dim3(drop_grid(n / 8)), dim3(DROP_THREADS), 0, stream, (const hcp_bf16*)dy, (const hcp_bf16*)nullptr,
               (hcp_bf16*)dx, n / 8, state, (uint32_t)layer_id, group_base, T, scale);
    HCP_LAUNCH_CHECK("dropout_bwd");
}

// state[1] += 1: the forward count of a module, once per training forward, before any layer runs.
HCP_API int hcp_dropout_advance(long long* state, hipStream_t stream) {
    HCP_REQUIRE(state, "hcp_dropout_advance: null state");
    HCP_LAUNCH(dropout_advance_kernel, dim3(1), dim3(64), 0, stream, state);
    HCP_LAUNCH_CHECK("dropout_advance");
}
