// noise.hip — the noise side of the training step beyond plain DDPM add_noise (reference hcpdiff/noise/pyramid_noise.py):
//
//  * pyramid (multi-resolution) noise   noise += resize(field_i -> (h, w)) * discount^i, i = 1..n_active, in ONE launch for all levels,
//                                       with ordered double partial sums (sum, sum of squares) of the result per workgroup
//  * its finish                         std over the whole tensor from the partials (fixed order, N - 1), then
//                                       xt = sqrt(acp[t_b]) x0 + sqrt(1 - acp[t_b]) noise / std
//
// The level sizes (hn, wn) and the level count are DEVICE data: a captured step replays one graph for every draw of the sizes.  Both
// launches are latency-bound (4*B*64*64 .. 4*B*128*128 elements), so a thread owns one output PIXEL and PYR_PL planes of it: the source
// coordinates and weights of a level are formed once per pixel and serve all of its planes, every tap of a level is requested before the
// first is used, and the taps of level i + 1 are requested before level i is consumed.  No atomics anywhere: the same bits on every run.
#include "hcp_common.h"

namespace {

constexpr int PYR_THREADS = 256;
constexpr int PYR_PL = 4;            // planes (b, c) per thread
constexpr int PYR_MAX = 16;          // HCP_PYRAMID_MAX_LEVELS
constexpr int PYR_PARTS = 4096;      // HCP_PYRAMID_PARTIALS: (sum, sumsq) pairs of workspace

struct PyrFields {
    const float* f[PYR_MAX];         // level i + 1: contiguous [B*C, hn, wn] at the start of f[i]
    long cap[PYR_MAX];               // elements f[i] holds
};

// what one pixel reads of one level: offsets inside a plane, the two bilinear weights, the plane's size
template <int NT> struct PyrTap {
    int o[NT];
    float ly, lx;
    int plane;
};

// F.interpolate(mode='bilinear', align_corners=False): src = max((dst + 0.5) in/out - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, in - 1)
HCP_DEVICE void pyr_axis_bilinear(int dst, int in, int out, int& i0, int& i1, float& l) {
    const float scale = (float)in / (float)out;
    float s = ((float)dst + 0.5f) * scale - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l = s - (float)i0;
    l = l < 0.f ? 0.f : (l > 1.f ? 1.f : l);
}
// F.interpolate(mode='nearest'): floor(dst * in/out)
HCP_DEVICE int pyr_axis_nearest(int dst, int in, int out) {
    if (in == out) return dst;
    int i = (int)floorf((float)dst * ((float)in / (float)out));
    return i > in - 1 ? in - 1 : i;
}

template <int MODE, int NT> HCP_DEVICE void pyr_setup(PyrTap<NT>& tp, int y, int x, int h, int w, int hn, int wn) {
    tp.plane = hn * wn;
    if (MODE == 0) {
        int y0, y1, x0, x1;
        pyr_axis_bilinear(y, hn, h, y0, y1, tp.ly);
        pyr_axis_bilinear(x, wn, w, x0, x1, tp.lx);
        tp.o[0] = y0 * wn + x0; tp.o[1 % NT] = y0 * wn + x1; tp.o[2 % NT] = y1 * wn + x0; tp.o[3 % NT] = y1 * wn + x1;
    } else {
        tp.ly = tp.lx = 0.f;
        tp.o[0] = pyr_axis_nearest(y, hn, h) * wn + pyr_axis_nearest(x, wn, w);
    }
}

template <int NT> HCP_DEVICE void pyr_load(float (&t)[PYR_PL][NT], const float* f, const PyrTap<NT>& tp, const int (&pc)[PYR_PL]) {
#pragma unroll
    for (int p = 0; p < PYR_PL; ++p) {
        const float* pl = f + (size_t)pc[p] * tp.plane;
#pragma unroll
        for (int k = 0; k < NT; ++k) t[p][k] = pl[tp.o[k]];
    }
}

HCP_DEVICE void pyr_block_sum2(double& a, double& b, double* red) {       // red [2][256]: a fixed tree, the same order on every run
    red[threadIdx.x] = a;
    red[PYR_THREADS + threadIdx.x] = b;
    HCP_SYNC();
    for (int k = PYR_THREADS / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) {
            red[threadIdx.x] += red[threadIdx.x + k];
            red[PYR_THREADS + threadIdx.x] += red[PYR_THREADS + threadIdx.x + k];
        }
        HCP_SYNC();
    }
    a = red[0]; b = red[PYR_THREADS];
    HCP_SYNC();
}

// grid (ceil(h w / 256), plane groups): workgroup (gx, gy) owns 256 pixels of the plane groups gy, gy + gridDim.y, ...
// A size table the field buffers cannot serve (hn or wn < 1, B C hn wn > cap) reads NOTHING and poisons the result with NaN.
template <int MODE> HCP_KERNEL(256) pyr_accum_kernel(float* noise, PyrFields F, int n_max, const int* dims, const int* n_active,
                                                      double discount, double* part, int BC, int h, int w, int groups) {
    constexpr int NT = MODE == 0 ? 4 : 1;
    HCP_DYN_SMEM(smem);
    double* red = (double*)smem;                                           // [2][256]
    int* sd = (int*)(smem + 2 * PYR_THREADS * sizeof(double));             // [2 * PYR_MAX]: (hn, wn) per level
    const int tid = threadIdx.x;
    if (tid < 2 * n_max) sd[tid] = dims[tid];
    HCP_SYNC();
    int n = *n_active;
    bool bad = n < 0 || n > n_max;
    if (bad) n = 0;
    for (int i = 0; i < n; ++i) {
        const int hn = sd[2 * i], wn = sd[2 * i + 1];
        if (hn < 1 || wn < 1 || hn > (1 << 15) || wn > (1 << 15) || (long)BC * hn * wn > F.cap[i]) bad = true;
    }
    if (bad) n = 0;
    const int hw = h * w;
    const int pix = blockIdx.x * PYR_THREADS + tid;
    const bool live = pix < hw;
    const int pq = live ? pix : 0;
    const int y = pq / w, x = pq - y * w;
    double s1 = 0.0, s2 = 0.0;
    for (int g = blockIdx.y; g < groups; g += gridDim.y) {
        int pc[PYR_PL];
        float v[PYR_PL];
#pragma unroll
        for (int p = 0; p < PYR_PL; ++p) {
            const int bc = g * PYR_PL + p;
            pc[p] = bc < BC ? bc : BC - 1;
            v[p] = noise[(size_t)pc[p] * hw + pq];
        }
        PyrTap<NT> cur, nxt;
        float tc[PYR_PL][NT], tn[PYR_PL][NT];
        if (n > 0) {
            pyr_setup<MODE, NT>(cur, y, x, h, w, sd[0], sd[1]);
            pyr_load<NT>(tc, F.f[0], cur, pc);
        }
        double dsc = 1.0;
        for (int i = 0; i < n; ++i) {
            if (i + 1 < n) {                                               // the next level's taps are in flight while this one is consumed
                pyr_setup<MODE, NT>(nxt, y, x, h, w, sd[2 * i + 2], sd[2 * i + 3]);
                pyr_load<NT>(tn, F.f[i + 1], nxt, pc);
            }
            dsc *= discount;                                               // discount**i in double, rounded once: torch's python scalar
            const float d = (float)dsc;
#pragma unroll
            for (int p = 0; p < PYR_PL; ++p) {
                float r;
                if (MODE == 0) {
                    const float top = (1.0f - cur.lx) * tc[p][0] + cur.lx * tc[p][1 % NT];
                    const float bot = (1.0f - cur.lx) * tc[p][2 % NT] + cur.lx * tc[p][3 % NT];
                    r = (1.0f - cur.ly) * top + cur.ly * bot;
                } else {
                    r = tc[p][0];
                }
                v[p] += r * d;
            }
            if (i + 1 < n) {
                cur = nxt;
#pragma unroll
                for (int p = 0; p < PYR_PL; ++p)
#pragma unroll
                    for (int k = 0; k < NT; ++k) tc[p][k] = tn[p][k];
            }
        }
#pragma unroll
        for (int p = 0; p < PYR_PL; ++p) {
            if (bad) v[p] = __builtin_nanf("");
            if (live && g * PYR_PL + p < BC) {
                noise[(size_t)pc[p] * hw + pq] = v[p];
                s1 += (double)v[p];
                s2 += (double)v[p] * (double)v[p];
            }
        }
    }
    pyr_block_sum2(s1, s2, red);
    if (tid == 0) {
        const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        part[2 * wg] = s1;
        part[2 * wg + 1] = s2;
    }
}

// Every workgroup adds the partials in the same fixed order (at most 4096 pairs from L2: cheaper than a launch of its own), then streams
// its share of xt.  vec: 16-byte loads / stores (per % 4 == 0: a vector never crosses a sample; 16-byte aligned buffers).
HCP_KERNEL(256) pyr_finish_kernel(const float* x0, const float* noise, const long long* t, const float* acp, float* xt,
                                  const double* part, int nparts, float* std_out, int B, long per, int vec) {
    HCP_DYN_SMEM(smem);
    double s1 = 0.0, s2 = 0.0;
    for (int k = threadIdx.x; k < nparts; k += PYR_THREADS) { s1 += part[2 * k]; s2 += part[2 * k + 1]; }
    pyr_block_sum2(s1, s2, (double*)smem);
    const double N = (double)B * (double)per;
    double var = (s2 - s1 * s1 / N) / (N - 1.0);                           // unbiased, as Tensor.std()
    var = var < 0.0 ? 0.0 : var;
    const float sd = (float)sqrt(var);
    if (std_out && blockIdx.x == 0 && threadIdx.x == 0) *std_out = sd;
    const long total = (long)B * per;
    if (vec) {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total / 4; i += (long)gridDim.x * blockDim.x) {
            const float a = acp[t[(i * 4) / per]];
            const float sa = sqrtf(a), sb = sqrtf(1.0f - a);
            const hcp_f32x4 xv = *(const hcp_f32x4*)(x0 + i * 4), nv = *(const hcp_f32x4*)(noise + i * 4);
            hcp_f32x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = sa * xv[q] + sb * (nv[q] / sd);
            *(hcp_f32x4*)(xt + i * 4) = o;
        }
    } else {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
            const float a = acp[t[i / per]];
            xt[i] = sqrtf(a) * x0[i] + sqrtf(1.0f - a) * (noise[i] / sd);
        }
    }
}

// the grid of the accumulate launch = the number of partial pairs the finish adds: a function of the shape alone
inline bool pyr_grid(int B, int C, int h, int w, int* gx, int* gy, int* groups) {
    const long hw = (long)h * w;
    const long x = (hw + PYR_THREADS - 1) / PYR_THREADS;
    if (x > PYR_PARTS) return false;
    const long gr = ((long)B * C + PYR_PL - 1) / PYR_PL;
    long y = PYR_PARTS / x;
    if (y > gr) y = gr;
    *gx = (int)x; *gy = (int)y; *groups = (int)gr;
    return true;
}

}  // namespace

// noise fp32 [B, C, h, w], in place: noise += resize(field_i -> (h, w)) * discount^i for i = 1 .. *n_active (<= n_max <= 16).
// fields: HOST array of n_max device pointers; field i is read as a contiguous [B, C, hn_i, wn_i] tensor at the start of its buffer of
// field_elems[i] floats (host array; the buffer may be larger than the level needs).  dims: device int32 [n_max][2] = (hn, wn);
// n_active: device int32.  mode 0 bilinear (align_corners = False), 1 nearest.  partials: 2 * HCP_PYRAMID_PARTIALS doubles.
HCP_API int hcp_pyramid_noise_accum(float* noise, const float* const* fields, const long* field_elems, int n_max, const int* dims,
                                    const int* n_active, double discount, int mode, double* partials, int B, int C, int h, int w,
                                    hipStream_t stream) {
    HCP_REQUIRE(noise && dims && n_active && partials && B > 0 && C > 0 && h > 0 && w > 0, "hcp_pyramid_noise_accum: bad arguments");
    HCP_REQUIRE(mode == 0 || mode == 1, "hcp_pyramid_noise_accum: resize mode %d: 0 (bilinear) or 1 (nearest)", mode);
    HCP_REQUIRE(n_max >= 0 && n_max <= PYR_MAX && (n_max == 0 || (fields && field_elems)),
                "hcp_pyramid_noise_accum: at most %d level fields", PYR_MAX);
    HCP_REQUIRE((long)B * C * h * w < (1L << 31) && (long)B * C * h * w >= 2, "hcp_pyramid_noise_accum: 2 <= B C h w < 2^31");
    PyrFields F;
    for (int i = 0; i < PYR_MAX; ++i) { F.f[i] = nullptr; F.cap[i] = 0; }
    for (int i = 0; i < n_max; ++i) {
        HCP_REQUIRE(fields[i] && field_elems[i] > 0, "hcp_pyramid_noise_accum: level field %d is null or empty", i + 1);
        F.f[i] = fields[i]; F.cap[i] = field_elems[i];
    }
    int gx, gy, groups;
    HCP_REQUIRE(pyr_grid(B, C, h, w, &gx, &gy, &groups), "hcp_pyramid_noise_accum: h w above %d", PYR_PARTS * PYR_THREADS);
    const size_t smem = 2 * PYR_THREADS * sizeof(double) + 2 * PYR_MAX * sizeof(int);
    if (mode == 0)
        HCP_LAUNCH(pyr_accum_kernel<0>, dim3(gx, gy), dim3(PYR_THREADS), smem, stream, noise, F, n_max, dims, n_active, discount, partials,
                   B * C, h, w, groups);
    else
        HCP_LAUNCH(pyr_accum_kernel<1>, dim3(gx, gy), dim3(PYR_THREADS), smem, stream, noise, F, n_max, dims, n_active, discount, partials,
                   B * C, h, w, groups);
    HCP_LAUNCH_CHECK("pyramid_noise_accum");
}

// std (unbiased, over all B C h w values) of the tensor hcp_pyramid_noise_accum left in `noise`, from its partials (same B, C, h, w), and
// xt = sqrt(acp[t_b]) x0 + sqrt(1 - acp[t_b]) noise / std.  `noise` itself is NOT normalised.  std_out: null or one device float.
HCP_API int hcp_pyramid_noise_finish(const float* x0, const float* noise, const long long* timesteps, const float* alphas_cumprod,
                                     float* xt, const double* partials, float* std_out, int B, int C, int h, int w, hipStream_t stream) {
    HCP_REQUIRE(x0 && noise && timesteps && alphas_cumprod && xt && partials && B > 0 && C > 0 && h > 0 && w > 0,
                "hcp_pyramid_noise_finish: bad arguments");
    HCP_REQUIRE((long)B * C * h * w < (1L << 31) && (long)B * C * h * w >= 2, "hcp_pyramid_noise_finish: 2 <= B C h w < 2^31");
    int gx, gy, groups;
    HCP_REQUIRE(pyr_grid(B, C, h, w, &gx, &gy, &groups), "hcp_pyramid_noise_finish: h w above %d", PYR_PARTS * PYR_THREADS);
    const long per = (long)C * h * w, total = (long)B * per;
    const int vec = per % 4 == 0 && (((size_t)x0 | (size_t)noise | (size_t)xt) & 15) == 0;
    long grid = ((vec ? total / 4 : total) + PYR_THREADS - 1) / PYR_THREADS;
    if (grid > 2048) grid = 2048;
    if (grid < 1) grid = 1;
    HCP_LAUNCH(pyr_finish_kernel, dim3((int)grid), dim3(PYR_THREADS), 2 * PYR_THREADS * sizeof(double), stream, x0, noise, timesteps,
               alphas_cumprod, xt, partials, gx * gy, std_out, B, per, vec);
    HCP_LAUNCH_CHECK("pyramid_noise_finish");
}
