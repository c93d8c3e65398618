// optim_factored.hip — the optimizers of the reference's SDXL full fine-tune and Lion examples on the flat fp32 buckets:
//   Lion      (lion_pytorch.Lion, cfgs/train/examples/Lion_optimizer.yaml): one elementwise launch, as AdamW in optim.hip;
//   Adafactor (transformers.optimization.Adafactor, cfgs/train/examples/FT_sdxl.yaml): factored second moments PER TENSOR, stepped for a
//             whole bucket from a descriptor table (one row per parameter) in three grouped passes + three small finish launches.
// Both take the conventions of adamw_kernel: global-norm clip / grad_scale prologue, device-resident lr and step counter, g left zero.
//
// Adafactor, per tensor (logical shape [.., R, C], factored over the last two dims; step t, beta2t = 1 - t^decay_rate):
//   s = g^2 + eps1;  row = beta2t row + (1 - beta2t) mean_C(s);  col = beta2t col + (1 - beta2t) mean_R(s)         (1-D: v likewise)
//   u = g rsqrt(row / mean_R(row)) rsqrt(col)    (1-D: g rsqrt(v));     u /= max(1, rms(u) / clip_threshold)
//   lr_t = max(eps2, rms(p)) [scale_parameter] * (lr | min(1e-2 or 1e-6 t, 1 / sqrt(t)) [relative_step])
//   upd = lr_t u;  [beta1: m = beta1 m + (1 - beta1) upd; upd = m];   p += -weight_decay lr_t p;   p -= upd
// Passes (each ONE launch over the bucket's work items; a work item = one workgroup's share of one tensor):
//   1 stats   reads g, p: row / column sums of s (MAT: per-tile partials to the workspace; TILE / VEC: the state itself), partial sum p^2
//   2 unorm   reads g + factors: partial sum u^2
//   3 apply   reads g, p (+ m), writes p (+ m), g = 0
// Every cross-workgroup sum is a set of per-work-item fp32 partials added in a fixed order by one thread or one workgroup: no
// floating-point atomic anywhere, the step is bit-reproducible.  Nothing is cleared, allocated or synchronised.
#include "hcp_common.h"

namespace {

enum { AF_VEC = 0, AF_MAT = 1, AF_TILE = 2 };
constexpr int AF_TR = 32;          // MAT tile: rows
constexpr int AF_TC = 1024;        // MAT tile: columns (256 threads x 4)
constexpr int AF_VEC_ITEM = 4096;  // VEC elements per work item (256 threads x 4 x 4)

struct AfDesc {                    // 112 bytes, mirrored by kernels.AF_DESC_DTYPE (numpy structured dtype)
    long off;                      // first element in the bucket (p, g, exp_avg share it)
    long row_off, col_off;         // MAT / TILE: offsets into the flat row / column second-moment buffers
    long full_off;                 // VEC: offset into the flat unfactored second-moment buffer
    long rowp_off, colp_off;       // MAT: offsets of the per-tile row / column partial sums in the workspace (floats)
    long s_outer, s_inner;         // element strides of the two outer dims (TILE: O and I), of R and of C
    long s_r, s_c;
    int kind;
    int outer, inner;              // TILE: O, I (outer positions = outer * inner); 1, 1 otherwise
    int R, C;                      // VEC: R = 1, C = numel
    int item0;                     // first work item of the three passes
    int fitem0;                    // first work item of the factor finish (MAT: ceil(max(R, C) / 256); 0 items otherwise)
    int pad_;
};
static_assert(sizeof(AfDesc) == 112, "descriptor layout is part of the ABI");

struct AfArgs {
    float* p; float* g; float* m;               // m: null without beta1
    float* row; float* col; float* full;
    const AfDesc* descs; int count;
    float* ws;                                  // [0, items): partial sums (p^2, then u^2); MAT tile partials behind them
    float* tstat;                               // per tensor: {rms(p), mean_R(row), lr_t, lr_t / max(1, rms(u) / clip_threshold)}
    float* scal;                                // {clip, beta2t, rel_step, -}: written by the prologue
    float eps1, eps2, clip_threshold, beta1, omb1, wd;      // omb1 = 1 - beta1, formed in double on the host
    int scale_parameter;
};

HCP_DEVICE float af_rsqrt(float x) {
#if defined(HCP_EMU)
    return 1.0f / sqrtf(x);
#else
    return rsqrtf(x);
#endif
}

// 4 elements p[0], p[stride], ..: one 16-byte access when `vec` (stride 1, aligned), else up to nvalid scalar ones (the rest read 0)
HCP_DEVICE hcp_f32x4 af_ld4(const float* p, long stride, int nvalid, bool vec) {
    if (vec) return *(const hcp_f32x4*)p;
    hcp_f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < 4; ++j) if (j < nvalid) v[j] = p[j * stride];
    return v;
}
HCP_DEVICE void af_st4(float* p, long stride, int nvalid, bool vec, hcp_f32x4 v) {
    if (vec) { *(hcp_f32x4*)p = v; return; }
    for (int j = 0; j < 4; ++j) if (j < nvalid) p[j * stride] = v[j];
}

// last descriptor whose first item is <= b (descriptors without items share their successor's first item and are skipped)
template <bool FIN> HCP_DEVICE int af_find(const AfDesc* d, int count, int b) {
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((FIN ? d[mid].fitem0 : d[mid].item0) <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// sum over the workgroup in a fixed order (butterfly inside a wave, waves 0..3 in order); valid in thread 0
HCP_DEVICE float af_block_sum(float v, float* red) {
    v = hcp_wave_sum(v);
    HCP_SYNC();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    HCP_SYNC();
    return red[0] + red[1] + red[2] + red[3];
}

// Step prologue (one thread): t += 1; clip factor of the global-norm clip; beta2t and the relative step in double, as the Python class
HCP_KERNEL(64) af_prologue_kernel(int* step, float* scal, const float* lr_p, const float* sumsq, float grad_scale, float max_norm,
                                  float decay_rate, int relative_step, int warmup_init) {
    if (threadIdx.x != 0) return;
    const int t = *step + 1;
    *step = t;
    float clip = grad_scale;
    if (sumsq && max_norm > 0.f) {
        const float norm = sqrtf(*sumsq) * grad_scale;
        const float c = max_norm / (norm + 1e-6f);
        if (c < 1.f) clip *= c;
    }
    scal[0] = clip;
    scal[1] = (float)(1.0 - pow((double)t, (double)decay_rate));
    double rel = lr_p ? (double)*lr_p : 0.0;
    if (relative_step) {
        const double min_step = warmup_init ? 1e-6 * (double)t : 1e-2;
        const double inv = 1.0 / sqrt((double)t);
        rel = min_step < inv ? min_step : inv;
    }
    scal[2] = (float)rel;
    scal[3] = 0.f;
}

// The three passes.  PASS 1: stats, 2: update norm, 3: apply.
template <int PASS> HCP_KERNEL(256) af_pass_kernel(AfArgs a) {
    HCP_DYN_SMEM(smem);
    float* red = (float*)smem;                  // [4]
    float* rsum = red + 4;                      // [AF_TR][4]  (MAT, pass 1)
    const int b = blockIdx.x, tid = threadIdx.x;
    const int ti = af_find<false>(a.descs, a.count, b);
    const AfDesc d = a.descs[ti];
    const int it = b - d.item0;
    const float clip = a.scal[0], b2 = a.scal[1];
    const float* ts = a.tstat + 4 * (long)ti;
    const float scale = PASS == 3 ? ts[3] : 0.f, lr_t = PASS == 3 ? ts[2] : 0.f;
    const float b1 = a.beta1, decay = -a.wd * lr_t;
    float* P = a.p + d.off; float* G = a.g + d.off; float* M = a.m ? a.m + d.off : nullptr;
    const bool base16 = ((((uintptr_t)P) | ((uintptr_t)G) | (M ? (uintptr_t)M : 0)) & 15) == 0;
    float acc = 0.f;                            // pass 1: sum p^2; pass 2: sum u^2

    // pass 3 on one quad: u -> parameter, first moment, cleared gradient
    auto apply4 = [&](long e, long stride, int nv, bool vec, hcp_f32x4 u) {
        hcp_f32x4 pq = af_ld4(P + e, stride, nv, vec), mq = {0.f, 0.f, 0.f, 0.f};
        if (M) mq = af_ld4(M + e, stride, nv, vec);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float upd = u[j] * scale;
            if (M) { mq[j] = b1 * mq[j] + a.omb1 * upd; upd = mq[j]; }
            float pj = pq[j];
            pj = pj + decay * pj;
            pq[j] = pj - upd;
        }
        af_st4(P + e, stride, nv, vec, pq);
        if (M) af_st4(M + e, stride, nv, vec, mq);
        af_st4(G + e, stride, nv, vec, hcp_f32x4{0.f, 0.f, 0.f, 0.f});
    };

    if (d.kind == AF_VEC) {
        float* V = a.full + d.full_off;
        const bool vec16 = base16 && ((((uintptr_t)V) & 15) == 0);
        const long n = d.C;
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            const long e = (long)it * AF_VEC_ITEM + ((long)k * 256 + tid) * 4;
            const long left = n - e;
            const int nv = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
            if (nv == 0) continue;
            const bool vec = vec16 && nv == 4;
            hcp_f32x4 gq = af_ld4(G + e, 1, nv, vec), vq = af_ld4(V + e, 1, nv, vec), u;
            if (PASS == 1) {
                const hcp_f32x4 pq = af_ld4(P + e, 1, nv, vec);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float gi = gq[j] * clip;
                    vq[j] = b2 * vq[j] + (1.f - b2) * (gi * gi + a.eps1);
                    acc += pq[j] * pq[j];
                }
                af_st4(V + e, 1, nv, vec, vq);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) { u[j] = j < nv ? gq[j] * clip * af_rsqrt(vq[j]) : 0.f; acc += u[j] * u[j]; }
                if (PASS == 3) apply4(e, 1, nv, vec, u);
            }
        }
    } else if (d.kind == AF_MAT) {
        const int nct = (d.C + AF_TC - 1) / AF_TC;
        const int rb = it / nct, cb = it % nct;
        const int r0 = rb * AF_TR, c = cb * AF_TC + tid * 4;
        const int nrow = d.R - r0 < AF_TR ? d.R - r0 : AF_TR;
        const int left = d.C - c;
        const int nv = left >= 4 ? 4 : (left > 0 ? left : 0);
        const bool vec = base16 && (d.C & 3) == 0 && nv == 4;
        float* row = a.row + d.row_off; float* col = a.col + d.col_off;
        hcp_f32x4 cacc = {0.f, 0.f, 0.f, 0.f}, cf = {0.f, 0.f, 0.f, 0.f};
        if (PASS != 1)
            for (int j = 0; j < 4; ++j) if (j < nv) cf[j] = af_rsqrt(col[c + j]);
        const float rmean = PASS != 1 ? ts[1] : 1.f;
#pragma unroll 1
        for (int r = 0; r < nrow; ++r) {
            const long e = (long)(r0 + r) * d.C + c;
            hcp_f32x4 gq = {0.f, 0.f, 0.f, 0.f};
            if (nv) gq = af_ld4(G + e, 1, nv, vec);
            if (PASS == 1) {
                float rs = 0.f;
                if (nv) {
                    const hcp_f32x4 pq = af_ld4(P + e, 1, nv, vec);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float gi = gq[j] * clip;
                        const float s = j < nv ? gi * gi + a.eps1 : 0.f;
                        cacc[j] += s; rs += s;
                        acc += pq[j] * pq[j];
                    }
                }
                rs = hcp_wave_sum(rs);
                if ((tid & 63) == 0) rsum[r * 4 + (tid >> 6)] = rs;
            } else {
                const float rf = af_rsqrt(row[r0 + r] / rmean);
                hcp_f32x4 u;
#pragma unroll
                for (int j = 0; j < 4; ++j) { u[j] = gq[j] * clip * rf * cf[j]; acc += u[j] * u[j]; }
                if (PASS == 3 && nv) apply4(e, 1, nv, vec, u);
            }
        }
        if (PASS == 1) {
            float* colp = a.ws + d.colp_off + (long)rb * d.C;
            for (int j = 0; j < 4; ++j) if (j < nv) colp[c + j] = cacc[j];
            HCP_SYNC();
            if (tid < nrow) a.ws[d.rowp_off + (long)(r0 + tid) * nct + cb] = rsum[tid * 4] + rsum[tid * 4 + 1] + rsum[tid * 4 + 2] + rsum[tid * 4 + 3];
        }
    } else {                                    // AF_TILE: a thread owns 4 consecutive inner positions of one outer row, all R x C taps
        const int nq = (d.inner + 3) / 4;
        const long quad = (long)it * 256 + tid;
        const int R = d.R, C = d.C;
        if (quad < (long)d.outer * nq) {
            const int o = (int)(quad / nq), i0 = (int)(quad % nq) * 4;
            const int nv = d.inner - i0 >= 4 ? 4 : d.inner - i0;
            const long e0 = (long)o * d.s_outer + (long)i0 * d.s_inner;
            const bool vec = base16 && d.s_inner == 1 && nv == 4 && ((e0 | d.s_outer | d.s_r | d.s_c) & 3) == 0;
            const long q0 = (long)o * d.inner + i0;
            float* row = a.row + d.row_off + q0 * R; float* col = a.col + d.col_off + q0 * C;
            hcp_f32x4 gq[9], rs[3], cs[3];      // R, C <= 3: every loop below is unrolled over 3 x 3 with a predicate, so these stay registers
#pragma unroll
            for (int k = 0; k < 3; ++k) rs[k] = cs[k] = hcp_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) {
                    if (r >= R || cc >= C) continue;
                    const long e = e0 + r * d.s_r + cc * d.s_c;
                    hcp_f32x4 v = af_ld4(G + e, d.s_inner, nv, vec);
                    if (PASS == 1) {
                        const hcp_f32x4 pq = af_ld4(P + e, d.s_inner, nv, vec);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float gi = v[j] * clip;
                            const float s = gi * gi + a.eps1;
                            rs[r][j] += s; cs[cc][j] += s;
                            acc += pq[j] * pq[j];
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] *= clip;
                        gq[r * 3 + cc] = v;
                    }
                }
            if (PASS == 1) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j >= nv) continue;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        if (k < R) row[j * R + k] = b2 * row[j * R + k] + (1.f - b2) * (rs[k][j] / (float)C);
                        if (k < C) col[j * C + k] = b2 * col[j * C + k] + (1.f - b2) * (cs[k][j] / (float)R);
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {   // factors of position j: rsqrt(row / mean_R(row)), rsqrt(col)
                    if (j >= nv) continue;
                    float rmean = 0.f;
#pragma unroll
                    for (int k = 0; k < 3; ++k) if (k < R) { rs[k][j] = row[j * R + k]; rmean += rs[k][j]; }
                    rmean /= (float)R;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        if (k < R) rs[k][j] = af_rsqrt(rs[k][j] / rmean);
                        if (k < C) cs[k][j] = af_rsqrt(col[j * C + k]);
                    }
                }
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int cc = 0; cc < 3; ++cc) {
                        if (r >= R || cc >= C) continue;
                        hcp_f32x4 u;
#pragma unroll
                        for (int j = 0; j < 4; ++j) { u[j] = j < nv ? gq[r * 3 + cc][j] * rs[r][j] * cs[cc][j] : 0.f; acc += u[j] * u[j]; }
                        if (PASS == 3) apply4(e0 + r * d.s_r + cc * d.s_c, d.s_inner, nv, vec, u);
                    }
            }
        }
    }
    if (PASS != 3) {
        const float s = af_block_sum(acc, red);
        if (tid == 0) a.ws[b] = s;
    }
}

// MAT tensors: the tile partials of pass 1 -> row / column moments.  Thread i of the tensor owns row i and column i; tiles are added in
// increasing tile order.
HCP_KERNEL(256) af_finish_factors_kernel(AfArgs a) {
    const int b = blockIdx.x;
    const int ti = af_find<true>(a.descs, a.count, b);
    const AfDesc d = a.descs[ti];
    const int idx = (b - d.fitem0) * 256 + threadIdx.x;
    const float b2 = a.scal[1];
    const int nct = (d.C + AF_TC - 1) / AF_TC, nrb = (d.R + AF_TR - 1) / AF_TR;
    if (idx < d.R) {
        const float* rp = a.ws + d.rowp_off + (long)idx * nct;
        float s = 0.f;
        for (int k = 0; k < nct; ++k) s += rp[k];
        float* row = a.row + d.row_off;
        row[idx] = b2 * row[idx] + (1.f - b2) * (s / (float)d.C);
    }
    if (idx < d.C) {
        const float* cp = a.ws + d.colp_off + idx;
        float s = 0.f;
        for (int k = 0; k < nrb; ++k) s += cp[(long)k * d.C];
        float* col = a.col + d.col_off;
        col[idx] = b2 * col[idx] + (1.f - b2) * (s / (float)d.R);
    }
}

// One workgroup per tensor.  phase 0 (after pass 1 + factor finish): rms(p), mean_R(row), lr_t.  phase 1 (after pass 2): the update scale.
HCP_KERNEL(256) af_finish_tensor_kernel(AfArgs a, int phase, int total_items) {
    HCP_DYN_SMEM(smem);
    float* red = (float*)smem;
    const int ti = blockIdx.x, tid = threadIdx.x;
    const AfDesc d = a.descs[ti];
    const int items = (ti + 1 < a.count ? a.descs[ti + 1].item0 : total_items) - d.item0;
    float acc = 0.f;
    for (int k = tid; k < items; k += 256) acc += a.ws[d.item0 + k];
    const float sum = af_block_sum(acc, red);
    const double numel = (double)d.outer * (double)d.inner * (double)d.R * (double)d.C;      // (one thread per tensor: the root in double)
    float* ts = a.tstat + 4 * (long)ti;
    if (phase == 0) {
        float racc = 0.f;
        if (d.kind == AF_MAT) {
            const float* row = a.row + d.row_off;
            for (int k = tid; k < d.R; k += 256) racc += row[k];
        }
        const float rsum = af_block_sum(racc, red);
        if (tid == 0) {
            const float rms = (float)sqrt((double)sum / numel);
            ts[0] = rms;
            ts[1] = d.kind == AF_MAT ? rsum / (float)d.R : 1.f;
            ts[2] = (a.scale_parameter ? fmaxf(a.eps2, rms) : 1.f) * a.scal[2];
        }
    } else if (tid == 0) {
        const float rms_u = (float)sqrt((double)sum / numel);
        ts[3] = ts[2] / fmaxf(1.f, rms_u / a.clip_threshold);
    }
}

// Sum of squares without atomics: one partial per workgroup, added in workgroup order by the finish (hcp_sumsq_f32 in optim.hip adds its
// block sums with fp32 atomics: the order, and with it the last bits of the clip factor, change from run to run).
HCP_KERNEL(256) sumsq_partial_kernel(const float* g, long n, float* part) {
    HCP_DYN_SMEM(smem);
    float acc = 0.f;
    const long n4 = ((((uintptr_t)g) & 15) == 0) ? n / 4 : 0;
    const hcp_f32x4* g4 = (const hcp_f32x4*)g;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const hcp_f32x4 v = g4[i];
        acc += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    for (long i = n4 * 4 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) acc += g[i] * g[i];
    const float s = af_block_sum(acc, (float*)smem);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}
HCP_KERNEL(256) sumsq_finish_kernel(const float* part, int count, float* out) {
    HCP_DYN_SMEM(smem);
    float acc = 0.f;
    for (int k = threadIdx.x; k < count; k += 256) acc += part[k];
    const float s = af_block_sum(acc, (float*)smem);
    if (threadIdx.x == 0) *out = s;
}

HCP_KERNEL(64) lion_step_inc_kernel(int* step) {
    if (threadIdx.x == 0) *step += 1;
}

HCP_DEVICE float lion_sign(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

HCP_KERNEL(256) lion_kernel(float* p, float* g, float* m, long n, const float* lr_p, float beta1, float omb1, float beta2, float omb2, float wd,
                            const float* sumsq, float grad_scale, float max_norm) {
    const float lr = *lr_p;
    float clip = grad_scale;
    if (sumsq && max_norm > 0.f) {
        const float norm = sqrtf(*sumsq) * grad_scale;
        const float c = max_norm / (norm + 1e-6f);
        if (c < 1.f) clip *= c;
    }
    const float decay = 1.f - lr * wd;
    const long n4 = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m) & 15) == 0) ? n / 4 : 0;
    hcp_f32x4* p4 = (hcp_f32x4*)p; hcp_f32x4* g4 = (hcp_f32x4*)g; hcp_f32x4* m4 = (hcp_f32x4*)m;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        hcp_f32x4 gq = g4[i], pq = p4[i], mq = m4[i];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float gi = gq[q] * clip;
            pq[q] = pq[q] * decay - lr * lion_sign(beta1 * mq[q] + omb1 * gi);
            mq[q] = beta2 * mq[q] + omb2 * gi;
        }
        p4[i] = pq; m4[i] = mq; g4[i] = hcp_f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (long i = n4 * 4 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float gi = g[i] * clip;
        p[i] = p[i] * decay - lr * lion_sign(beta1 * m[i] + omb1 * gi);
        m[i] = beta2 * m[i] + omb2 * gi;
        g[i] = 0.f;
    }
}

}  // namespace

// Lion (lion_pytorch semantics) on a flat bucket: g *= grad_scale, global-norm clip as hcp_adamw_clip_fused, then
// p *= 1 - lr wd;  p -= lr sign(beta1 m + (1 - beta1) g)  (sign(0) = 0);  m = beta2 m + (1 - beta2) g;  g = 0.  *step is incremented.
// The betas arrive as doubles: 1 - beta is formed in double and rounded once (1.f - 0.99f is off by 1e-6 of itself).
HCP_API int hcp_lion_clip_fused(float* p, float* g, float* m, long n, const float* lr, double beta1, double beta2, float weight_decay,
                                const float* sumsq, float grad_scale, float max_norm, int* step, hipStream_t stream) {
    HCP_REQUIRE(p && g && m && lr && step && n > 0, "hcp_lion_clip_fused: bad arguments");
    long grid = (n + 255) / 256; if (grid > 2048) grid = 2048;
    HCP_LAUNCH(lion_step_inc_kernel, dim3(1), dim3(64), 0, stream, step);
    HCP_LAUNCH(lion_kernel, dim3((int)grid), dim3(256), 0, stream, p, g, m, n, lr, (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
               weight_decay, sumsq, grad_scale, max_norm);
    HCP_LAUNCH_CHECK("lion_clip_fused");
}

// out[0] = sum(g^2), bit-reproducible: `partials` holds one float per workgroup (HCP_SUMSQ_PARTIALS = 2048 floats always suffice)
HCP_API int hcp_sumsq_ordered_f32(const float* g, long n, float* out, float* partials, hipStream_t stream) {
    HCP_REQUIRE(g && out && partials && n > 0, "hcp_sumsq_ordered_f32: bad arguments");
    long grid = (n + 4095) / 4096;
    if (grid > 2048) grid = 2048;
    HCP_LAUNCH(sumsq_partial_kernel, dim3((int)grid), dim3(256), 4 * sizeof(float), stream, g, n, partials);
    HCP_LAUNCH(sumsq_finish_kernel, dim3(1), dim3(256), 4 * sizeof(float), stream, (const float*)partials, (int)grid, out);
    HCP_LAUNCH_CHECK("sumsq_ordered");
}

HCP_API int hcp_adafactor_desc_bytes(void) { return (int)sizeof(AfDesc); }

// One Adafactor step over the `count` tensors of a flat bucket (descs: device array of AfDesc sorted by item0, built by
// kernels.adafactor_table).  m: first moments (null = beta1 None); row / col / full: flat second-moment state; workspace: the floats
// the table asks for (work-item partials + MAT tile partials); tstat: 4 floats per tensor; scal: 4 floats.  lr: device scalar (null with
// relative_step).  Seven launches whatever the number of tensors.
HCP_API int hcp_adafactor_step(float* p, float* g, float* m, float* row, float* col, float* full, const void* descs, int count,
                               int total_items, int total_fitems, float* workspace, size_t workspace_bytes, float* tstat, float* scal,
                               const float* lr, float eps1, float eps2, float clip_threshold, float decay_rate, double beta1,
                               float weight_decay, int scale_parameter, int relative_step, int warmup_init, const float* sumsq,
                               float grad_scale, float max_norm, int* step, hipStream_t stream) {
    HCP_REQUIRE(p && g && descs && workspace && tstat && scal && step && count > 0 && total_items >= count && total_fitems >= 0,
                "hcp_adafactor_step: bad arguments");
    HCP_REQUIRE(workspace_bytes >= (size_t)total_items * sizeof(float), "hcp_adafactor_step: workspace too small");
    HCP_REQUIRE(lr || relative_step, "hcp_adafactor_step: lr is required without relative_step");
    HCP_REQUIRE(clip_threshold > 0.f, "hcp_adafactor_step: clip_threshold must be positive");
    AfArgs a;
    a.p = p; a.g = g; a.m = m; a.row = row; a.col = col; a.full = full;
    a.descs = (const AfDesc*)descs; a.count = count; a.ws = workspace; a.tstat = tstat; a.scal = scal;
    a.eps1 = eps1; a.eps2 = eps2; a.clip_threshold = clip_threshold; a.beta1 = (float)beta1; a.omb1 = (float)(1.0 - beta1); a.wd = weight_decay; a.scale_parameter = scale_parameter;
    const size_t smem = (4 + AF_TR * 4) * sizeof(float);
    HCP_LAUNCH(af_prologue_kernel, dim3(1), dim3(64), 0, stream, step, scal, lr, sumsq, grad_scale, max_norm, decay_rate, relative_step, warmup_init);
    HCP_LAUNCH(af_pass_kernel<1>, dim3(total_items), dim3(256), smem, stream, a);
    if (total_fitems > 0) HCP_LAUNCH(af_finish_factors_kernel, dim3(total_fitems), dim3(256), 0, stream, a);
    HCP_LAUNCH(af_finish_tensor_kernel, dim3(count), dim3(256), smem, stream, a, 0, total_items);
    HCP_LAUNCH(af_pass_kernel<2>, dim3(total_items), dim3(256), smem, stream, a);
    HCP_LAUNCH(af_finish_tensor_kernel, dim3(count), dim3(256), smem, stream, a, 1, total_items);
    HCP_LAUNCH(af_pass_kernel<3>, dim3(total_items), dim3(256), smem, stream, a);
    HCP_LAUNCH_CHECK("adafactor_step");
}
