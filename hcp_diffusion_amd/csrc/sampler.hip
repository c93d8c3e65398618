// sampler.hip — Euler / Euler-ancestral sampling (the k-diffusion update diffusers' EulerAncestralDiscreteScheduler and
// EulerDiscreteScheduler publish, epsilon prediction) fused with classifier-free guidance, the inpaint blend of the reference's legacy
// pipeline (utils/pipe_hook.py:429,442,453) and the next UNet input, ONE launch per sampling step.
//
// Nothing that varies per step is a kernel argument.  A run owns two device tensors:
//   table  float[steps][8], built on the host in float64 and rounded once.  Row i:
//            0 sigma_i   1 sigma_down_i   2 sigma_up_i   3 c_in_next_i = 1 / sqrt(sigma_next_i^2 + 1)   4 timestep_i   5 timestep_next_i
//            6 sigma_init_i (what a text2img run that STARTS at row i scales its unit noise by)   7 c_in_i = 1 / sqrt(sigma_i^2 + 1)
//          The last row of a run has sigma_next = 0, hence sigma_down = sigma_up = 0 and c_in_next = 1: sigma_down == 0 IS the mark of the
//          final step (sigma_down^2 = sigma_next^4 / sigma^2 vanishes with sigma_next only).  Plain Euler: sigma_up = 0, sigma_down = sigma_next.
//   state  int64[2] = (seed, step).  hcp_sampler_begin sets step, hcp_sampler_advance bumps it (its own launch, so no block of the step
//          kernel races the increment), the step kernel reads row state[1] (clamped into the table).
// So one captured graph {UNet forward, hcp_euler_step, hcp_sampler_advance} serves every step of every run on the same buffers.
//
// Ancestral noise, when no tensor is given: element group g (four consecutive elements, one 16-byte access) draws Philox4x32-10 with
//   counter = (lo32(g), hi32(g), lo32(step), 0x53414D50 "SAMP"),  key = (lo32(seed), hi32(seed));
// u_j = (w_j + 0.5) * 2^-32 in (0, 1], two Box-Muller pairs: z0, z1 = sqrt(-2 ln u0) (cos, sin)(2 pi u1), z2, z3 likewise from u2, u3.
// hcp_sampler_begin's own draw (no noise tensor) uses step word 0xFFFFFFFF, which no run reaches.  No noise is drawn when sigma_up == 0.
// Grid-stride over groups, 16-byte loads and stores, no atomics, no workspace; x_out may alias x (a thread reads its 16 bytes before it
// writes them).  The step kernel is launch-latency bound (B = 4 at 64 x 64 is 65 536 floats): what it buys is the loop around it.
#include "hcp_common.h"
#include "hcp_philox.h"
#include <math.h>

// Every product and sum below is rounded on its own: a caller that does the guidance combine itself (scheduler.NativeEulerAncestralScheduler
// under the reference's loop) and the fused form then give the same bits.
#pragma clang fp contract(off)

namespace {

constexpr int SMP_THREADS = 256;
constexpr long SMP_MAX_BLOCKS = 512;            // kernels.SAMPLER_MAX_THREADS = SMP_MAX_BLOCKS * SMP_THREADS
constexpr int SMP_ROW = 8;                      // floats per table row
constexpr uint32_t SMP_TAG = 0x53414D50u;
constexpr uint32_t SMP_BEGIN_STEP = 0xFFFFFFFFu;
inline int smp_grid(long groups) {
    long g = (groups + SMP_THREADS - 1) / SMP_THREADS;
    if (g > SMP_MAX_BLOCKS) g = SMP_MAX_BLOCKS;
    if (g < 1) g = 1;
    return (int)g;
}

HCP_DEVICE hcp_f32x4 smp_normal4(unsigned long long group, uint32_t step, uint32_t k0, uint32_t k1) {
    uint32_t w[4];
    philox4x32_10((uint32_t)group, (uint32_t)(group >> 32), step, SMP_TAG, k0, k1, w);
    float u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = ((float)w[j] + 0.5f) * 2.3283064365386963e-10f;
    const float r0 = sqrtf(-2.0f * logf(u[0])), r1 = sqrtf(-2.0f * logf(u[2]));
    const float a0 = 6.2831853071795865f * u[1], a1 = 6.2831853071795865f * u[3];
    hcp_f32x4 z;
    z[0] = r0 * cosf(a0); z[1] = r0 * sinf(a0);
    z[2] = r1 * cosf(a1); z[3] = r1 * sinf(a1);
    return z;
}

HCP_DEVICE long smp_row(const long long* state, int steps) {
    long s = (long)state[1];
    return s < 0 ? 0 : (s >= steps ? steps - 1 : s);
}

HCP_KERNEL(256) euler_step_kernel(const float* x, const float* eps2, float* x_out, float* model_in_next, long groups, long cond_off,
                                  float guidance, const float* table, int steps, const long long* state, const float* noise,
                                  const float* init, const float* noise0, const float* mask, long chw, long hw) {
    const unsigned long long seed = (unsigned long long)state[0];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const long row = smp_row(state, steps);
    const float* r = table + row * SMP_ROW;
    const float sigma = r[0], sigma_down = r[1], sigma_up = r[2], c_in_next = r[3];
    const float d = sigma_down - sigma;
    const bool last = sigma_down == 0.0f;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
        const long i = g * 4;
        const hcp_f32x4 xv = *(const hcp_f32x4*)(x + i);
        hcp_f32x4 e = *(const hcp_f32x4*)(eps2 + i);
        if (cond_off) {
            const hcp_f32x4 ec = *(const hcp_f32x4*)(eps2 + cond_off + i);
#pragma unroll
            for (int q = 0; q < 4; ++q) e[q] = e[q] + guidance * (ec[q] - e[q]);
        }
        hcp_f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = xv[q] + e[q] * d;
        if (sigma_up != 0.0f) {
            const hcp_f32x4 z = noise ? *(const hcp_f32x4*)(noise + i) : smp_normal4((unsigned long long)g, (uint32_t)row, k0, k1);
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = o[q] + z[q] * sigma_up;
        }
        if (mask) {
            const hcp_f32x4 iv = *(const hcp_f32x4*)(init + i), nv = *(const hcp_f32x4*)(noise0 + i);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long j = i + q;
                const float m = mask[(j / chw) * hw + j % hw];
                const float keep = last ? iv[q] : iv[q] + sigma * nv[q];       // the sigma of the step just taken (pipe_hook.py:442)
                o[q] = m * keep + (1.0f - m) * o[q];
            }
        }
        *(hcp_f32x4*)(x_out + i) = o;
        if (model_in_next) {
            hcp_f32x4 s;
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q] = c_in_next * o[q];
            *(hcp_f32x4*)(model_in_next + i) = s;
            if (cond_off) *(hcp_f32x4*)(model_in_next + cond_off + i) = s;
        }
    }
}

// state[1] <- min(state[1] + 1, steps - 1); t_out[0..rows) <- timestep of the new row.  One block of 64 threads: every thread reads the
// old count before the barrier, thread 0 writes the new one after it.
HCP_KERNEL(64) sampler_advance_kernel(long long* state, const float* table, int steps, long long* t_out, int rows) {
    long s = (long)state[1] + 1;
    s = s < 0 ? 0 : (s >= steps ? steps - 1 : s);
    HCP_SYNC();
    if (threadIdx.x == 0) state[1] = s;
    const long long t = (long long)table[s * SMP_ROW + 4];
    for (int j = threadIdx.x; j < rows; j += blockDim.x) t_out[j] = t;
}

// x <- (init +) z * scale, model_in <- c_in x; block 0 also sets state[1] and t_out.  z = noise[i] (may alias x) or the begin draw.
HCP_KERNEL(256) sampler_begin_kernel(long long* state, const float* table, float* x, float* model_in, long groups, long cond_off,
                                     const float* noise, const float* init, long long* t_out, int rows, int start_step) {
    const unsigned long long seed = (unsigned long long)state[0];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const float* r = table + (long)start_step * SMP_ROW;
    const float scale = init ? r[0] : r[6], c_in = r[7];
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) state[1] = start_step;
        const long long t = (long long)r[4];
        for (int j = threadIdx.x; j < rows; j += blockDim.x) t_out[j] = t;
    }
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
        const long i = g * 4;
        const hcp_f32x4 z = noise ? *(const hcp_f32x4*)(noise + i) : smp_normal4((unsigned long long)g, SMP_BEGIN_STEP, k0, k1);
        hcp_f32x4 o, s;
        if (init) {
            const hcp_f32x4 iv = *(const hcp_f32x4*)(init + i);
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = iv[q] + z[q] * scale;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = z[q] * scale;
        }
        *(hcp_f32x4*)(x + i) = o;
        if (model_in) {
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q] = c_in * o[q];
            *(hcp_f32x4*)(model_in + i) = s;
            if (cond_off) *(hcp_f32x4*)(model_in + cond_off + i) = s;
        }
    }
}

inline bool smp_aligned(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr, const void* e = nullptr,
                        const void* f = nullptr, const void* g = nullptr) {
    return (((size_t)a | (size_t)b | (size_t)c | (size_t)d | (size_t)e | (size_t)f | (size_t)g) & 15) == 0;
}

}  // namespace

// One Euler / Euler-ancestral step on row state[1] of `table` (layout above):
//   eps = eps2[:n] + guidance (eps2[n:] - eps2[:n]) when guided (eps2 = UNet output on [uncond ; cond]), else eps2[:n]
//   x'  = x + eps (sigma_down - sigma) + z sigma_up,  z = noise[i] or the in-kernel draw (none when sigma_up == 0)
//   mask (with init and noise0; [B_rows,1,h,w] broadcast over chw / hw channels): x' = m (init + sigma noise0) + (1 - m) x', on the final
//   row m init + (1 - m) x'
//   x_out = x' (may alias x);  model_in_next (nullable) [i] and, guided, [n + i] = c_in_next x'.
HCP_API int hcp_euler_step(const float* x, const float* eps2, float* x_out, float* model_in_next, long n, int B_rows, int guided,
                           float guidance, const float* table, int steps, const long long* state, const float* noise, const float* init,
                           const float* noise0, const float* mask, long chw, long hw, hipStream_t stream) {
    HCP_REQUIRE(table && state, "hcp_euler_step: null table or state");
    HCP_REQUIRE(steps > 0, "hcp_euler_step: steps must be positive");
    HCP_REQUIRE(x && eps2 && x_out, "hcp_euler_step: null x, eps2 or x_out");
    HCP_REQUIRE(n > 0 && n % 4 == 0, "hcp_euler_step: n must be a positive multiple of 4");
    HCP_REQUIRE(!mask || (init && noise0), "hcp_euler_step: a mask needs init and noise0");
    HCP_REQUIRE(!mask || (B_rows > 0 && hw > 0 && chw > 0 && chw % hw == 0 && n == (long)B_rows * chw),
                "hcp_euler_step: a mask needs n == B_rows * chw and chw a multiple of hw");
    HCP_REQUIRE(smp_aligned(x, eps2, x_out, model_in_next, noise, init, noise0), "hcp_euler_step: buffers must be 16-byte aligned");
    HCP_LAUNCH(euler_step_kernel, dim3(smp_grid(n / 4)), dim3(SMP_THREADS), 0, stream, x, eps2, x_out, model_in_next, n / 4,
               guided ? n : 0L, guidance, table, steps, state, noise, mask ? init : (const float*)nullptr,
               mask ? noise0 : (const float*)nullptr, mask, chw, hw);
    HCP_LAUNCH_CHECK("euler_step");
}

// state[1] <- min(state[1] + 1, steps - 1) and t_out[0..rows) <- the new row's timestep: once per sampling step, after hcp_euler_step.
HCP_API int hcp_sampler_advance(long long* state, const float* table, int steps, long long* t_out, int rows, hipStream_t stream) {
    HCP_REQUIRE(table && state, "hcp_sampler_advance: null table or state");
    HCP_REQUIRE(steps > 0, "hcp_sampler_advance: steps must be positive");
    HCP_REQUIRE(t_out && rows > 0, "hcp_sampler_advance: null t_out or no rows");
    HCP_LAUNCH(sampler_advance_kernel, dim3(1), dim3(64), 0, stream, state, table, steps, t_out, rows);
    HCP_LAUNCH_CHECK("sampler_advance");
}

// Start of a run at row start_step: state[1] <- start_step, t_out <- its timestep, x <- z sigma_init (text2img) or init + z sigma
// (img2img), z = noise[i] (may be x itself) or drawn here; model_in (nullable) [i] and, guided, [n + i] = c_in x.
HCP_API int hcp_sampler_begin(long long* state, const float* table, int steps, float* x, float* model_in, long n, int guided,
                              const float* noise, const float* init, long long* t_out, int rows, int start_step, hipStream_t stream) {
    HCP_REQUIRE(table && state, "hcp_sampler_begin: null table or state");
    HCP_REQUIRE(steps > 0, "hcp_sampler_begin: steps must be positive");
    HCP_REQUIRE(start_step >= 0 && start_step < steps, "hcp_sampler_begin: start_step outside the table");
    HCP_REQUIRE(x && t_out && rows > 0, "hcp_sampler_begin: null x or t_out, or no rows");
    HCP_REQUIRE(n > 0 && n % 4 == 0, "hcp_sampler_begin: n must be a positive multiple of 4");
    HCP_REQUIRE(smp_aligned(x, model_in, noise, init), "hcp_sampler_begin: buffers must be 16-byte aligned");
    HCP_LAUNCH(sampler_begin_kernel, dim3(smp_grid(n / 4)), dim3(SMP_THREADS), 0, stream, state, table, x, model_in, n / 4,
               guided ? n : 0L, noise, init, t_out, rows, start_step);
    HCP_LAUNCH_CHECK("sampler_begin");
}
