// embedding.hip — prompt tuning: the CLIP token embedding with trainable custom words (the reference's EmbeddingPTHook,
// hcpdiff/models/text_emb_ex.py:33-69, followed by CLIPTextEmbeddings' position add).
//
//  * forward:  ids [b, r*w] (the hook's regrouped layout) -> bf16 [b*r, n_word + 2, C].  Per batch item every id at or above `vocab`
//              that has a registered word is replaced by that word's n_vec custom vectors (the sequence shifts right), rows
//              [1, r*n_word + 1) of the expanded sequence are cut into r chunks of n_word rows, and each chunk gets BOS / EOS = the
//              token rows of ids[0][0] / ids[0][r*w - 1] (batch item 0, clipped ids, for every item).  Then + position row, in fp32,
//              rounded once to bf16.  A second output, the int32 source map [b*r, n_word + 2], records where every row came from
//              (>= 0: token-table row; < 0: custom row -1 - code) — the backward reads nothing else.
//  * backward: d custom[k, :] = sum of dX over the rows whose source is custom row k, in increasing row order (one workgroup per
//              (custom row, 256-column slab): no atomics, bit-reproducible), written or added (beta 0 / 1).
//
// Ids at or above `vocab` without a registered word (map entry absent, n_vec <= 0, or outside the custom table) and negative ids read
// the clipped token row, as the reference's table lookup does before its hook replaces the row; nothing is ever read out of bounds.
//
// Second half of the file: the other end of the text encoder — the pooled projection of CLIPTextModelWithProjection (clip_pool_*).
#include "hcp_common.h"

namespace {

constexpr int PT_THREADS = 256;
constexpr int PT_MAX_IDS = 2048;        // r*w ids of one batch item, and r*(n_word + 2) output rows, each held in LDS
constexpr int PT_BWD_CHUNK = 1024;      // source-map entries staged in LDS per pass of the backward

HCP_DEVICE int pt_clip(long long id, int vocab) { return id < 0 ? 0 : (id >= vocab ? vocab - 1 : (int)id); }

HCP_KERNEL(256) embedding_pt_fwd_kernel(const long long* ids, int R, int W, int n_word, const float* tok, int vocab, const float* pos,
                                        const long long* pos_ids, int n_pos, const float* cust, int n_cust, const int* cmap, int n_map,
                                        hcp_bf16* out, int* src_map, int C) {
    HCP_DYN_SMEM(smem);
    int* wid = (int*)smem;                       // [PT_MAX_IDS] width of every id (1, or n_vec of a custom word)
    int* start = wid + PT_MAX_IDS;               // [PT_MAX_IDS] exclusive prefix sum of wid = first expanded row of the id
    int* src0 = start + PT_MAX_IDS;              // [PT_MAX_IDS] source code of that first row
    int* rowsrc = src0 + PT_MAX_IDS;             // [PT_MAX_IDS] source code of every output row of this item
    int* part = rowsrc + PT_MAX_IDS;             // [2][PT_THREADS] per-thread chunk sums, ping-pong scan
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = R * W, WO = n_word + 2;
    const long long* my = ids + (size_t)b * n;
    for (int i = tid; i < n; i += PT_THREADS) {
        const long long id = my[i];
        int w = 1, s = pt_clip(id, vocab);
        if (id >= vocab && id - vocab < n_map) {
            const int off = cmap[2 * (id - vocab)], nv = cmap[2 * (id - vocab) + 1];
            if (nv > 0 && off >= 0 && off + nv <= n_cust) { w = nv; s = -1 - off; }
        }
        wid[i] = w; src0[i] = s;
    }
    HCP_SYNC();
    // exclusive scan: thread t owns ids [t*per, t*per + per); Hillis-Steele over the 256 chunk sums
    const int per = (n + PT_THREADS - 1) / PT_THREADS;
    const int lo = tid * per, hi = lo + per < n ? lo + per : n;
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += wid[i];
    part[tid] = sum;
    HCP_SYNC();
    int cur = 0;
    for (int d = 1; d < PT_THREADS; d <<= 1) {
        const int* src = part + cur * PT_THREADS;
        part[(cur ^ 1) * PT_THREADS + tid] = src[tid] + (tid >= d ? src[tid - d] : 0);
        cur ^= 1;
        HCP_SYNC();
    }
    int run = part[cur * PT_THREADS + tid] - sum;
    for (int i = lo; i < hi; ++i) { start[i] = run; run += wid[i]; }
    HCP_SYNC();
    // resolve every output row: BOS, r*n_word expanded rows starting at expanded row 1, EOS.  The expanded sequence is >= n rows long and
    // the host requires n >= r*n_word + 1, so the binary search always lands inside it.
    const int bos = pt_clip(ids[0], vocab), eos = pt_clip(ids[n - 1], vocab);
    for (int q = tid; q < R * WO; q += PT_THREADS) {
        const int k = q / WO, j = q - k * WO;
        int s;
        if (j == 0) s = bos;
        else if (j == WO - 1) s = eos;
        else {
            const int e = 1 + k * n_word + (j - 1);
            int l = 0, h = n - 1;                // largest i with start[i] <= e
            while (l < h) {
                const int m = (l + h + 1) >> 1;
                if (start[m] <= e) l = m; else h = m - 1;
            }
            s = src0[l];
            if (s < 0) s -= e - start[l];        // custom row off + (e - start): code -1 - off - (e - start)
        }
        rowsrc[q] = s;
        src_map[((size_t)b * R) * WO + q] = s;
    }
    HCP_SYNC();
    // gather: 8 columns per thread, two 16-byte fp32 loads from the source row and two from the position row, one 16-byte bf16 store
    const int cv = C / 8;
    for (int i = tid; i < R * WO * cv; i += PT_THREADS) {
        const int q = i / cv, c = (i - q * cv) * 8;
        const int k = q / WO, j = q - k * WO;
        const int s = rowsrc[q];
        const float* a = s >= 0 ? tok + (size_t)s * C + c : cust + (size_t)(-1 - s) * C + c;
        long long p = pos_ids ? pos_ids[((size_t)b * R + k) * WO + j] : j;
        p = p < 0 ? 0 : (p >= n_pos ? n_pos - 1 : p);
        const float* pp = pos + (size_t)p * C + c;
        const hcp_f32x4 a0 = *(const hcp_f32x4*)a, a1 = *(const hcp_f32x4*)(a + 4);
        const hcp_f32x4 p0 = *(const hcp_f32x4*)pp, p1 = *(const hcp_f32x4*)(pp + 4);
        hcp_bf16x8 o;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            o[t] = (short)hcp_f2bf(a0[t] + p0[t]);
            o[t + 4] = (short)hcp_f2bf(a1[t] + p1[t]);
        }
        *(hcp_bf16x8*)(out + (((size_t)b * R + k) * WO + j) * C + c) = o;
    }
}

HCP_KERNEL(256) embedding_pt_bwd_kernel(const hcp_bf16* dx, const int* src_map, long M, int C, float* grad, int beta) {
    HCP_DYN_SMEM(smem);
    int* codes = (int*)smem;                     // [PT_BWD_CHUNK]
    const int row = blockIdx.x, tid = threadIdx.x;
    const int col = blockIdx.y * PT_THREADS + tid;
    const int code = -1 - row;
    float acc = 0.0f;
    for (long m0 = 0; m0 < M; m0 += PT_BWD_CHUNK) {
        const int cnt = M - m0 < PT_BWD_CHUNK ? (int)(M - m0) : PT_BWD_CHUNK;
        for (int i = tid; i < cnt; i += PT_THREADS) codes[i] = src_map[m0 + i];
        HCP_SYNC();
        for (int i = 0; i < cnt; ++i)            // the same LDS word for every lane: a uniform branch, rows summed in increasing order
            if (codes[i] == code && col < C) acc += hcp_bf2f(dx[(size_t)(m0 + i) * C + col]);
        HCP_SYNC();
    }
    if (col < C) {
        float* g = grad + (size_t)row * C + col;
        *g = beta ? *g + acc : acc;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Pooled projection of CLIPTextModelWithProjection (SDXL's second encoder): text_projection(final_layer_norm(last_hidden)[eos]),
// averaged over the r chunks of one prompt (TEEXHook.forward_hook, textencoder_ex.py:73-76).  B*r is a handful of rows: a GEMV per
// prompt.  The projection is linear, so the r normalised EOS tokens are averaged FIRST (fp32, in LDS) and multiplied once.
//  * forward:  workgroup (prompt b, 16 output columns).  Per chunk: first position of the maximum id (transformers' rule for
//              eos_token_id == 2), two-pass LayerNorm statistics of that one token, xbar += LN(token) / r.  Then each wave forms its
//              columns' dot products with 16-byte weight loads and a wave sum.  Every output is written by exactly one lane.
//  * backward: workgroup = one row m = b*r + k.  g = W^T d_pooled[b] / r (8 partial sums over P per column, added in a fixed order),
//              LayerNorm backward of g at the EOS token, and the rest of dx[m] is cleared by the same workgroup: dx is WRITTEN.
constexpr int CP_THREADS = 256;
constexpr int CP_PSLICE = 16;
constexpr int CP_MAX = 8192;

HCP_DEVICE float cp_block_sum(float v, float* red) {
    v = hcp_wave_sum(v);
    HCP_SYNC();                                  // red may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    HCP_SYNC();
    return red[0] + red[1] + red[2] + red[3];
}

// first position of the maximum of ids[0, L): the same value in every thread
HCP_DEVICE int cp_first_argmax(const long long* ids, int L, long long* sv, int* si) {
    const int tid = threadIdx.x;
    long long best = 0; int bi = 0x7fffffff;
    for (int i = tid; i < L; i += CP_THREADS) {  // increasing i: a strict > keeps the first
        const long long v = ids[i];
        if (bi == 0x7fffffff || v > best) { best = v; bi = i; }
    }
    sv[tid] = best; si[tid] = bi;
    HCP_SYNC();
    for (int s = CP_THREADS / 2; s >= 1; s >>= 1) {
        if (tid < s) {
            const long long o = sv[tid + s]; const int oi = si[tid + s];
            const bool mine = si[tid] != 0x7fffffff;
            if (oi != 0x7fffffff && (!mine || o > sv[tid] || (o == sv[tid] && oi < si[tid]))) { sv[tid] = o; si[tid] = oi; }
        }
        HCP_SYNC();
    }
    const int r = si[0];
    HCP_SYNC();
    return r;
}

HCP_DEVICE void cp_load_w8(const void* W, int w_f32, size_t off, float (&w)[8]) {
    if (w_f32) {
        const hcp_f32x4 a = *(const hcp_f32x4*)((const float*)W + off), b = *(const hcp_f32x4*)((const float*)W + off + 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) { w[q] = a[q]; w[q + 4] = b[q]; }
    } else {
        const hcp_bf16x8 v = *(const hcp_bf16x8*)((const hcp_bf16*)W + off);
#pragma unroll
        for (int q = 0; q < 8; ++q) w[q] = hcp_bf2f((unsigned short)v[q]);
    }
}

HCP_KERNEL(256) clip_pool_fwd_kernel(const hcp_bf16* x, const long long* ids, const float* gamma, const float* beta, const void* W,
                                     int w_f32, float* pooled, int* pos_out, float* stats, int R, int L, int C, int P, float eps) {
    HCP_DYN_SMEM(smem);
    float* xbar = (float*)smem;                  // [C] mean over the chunks of LN(eos token)
    float* red = xbar + C;                       // [4]
    long long* sv = (long long*)(red + 4);       // [CP_THREADS]
    int* si = (int*)(sv + CP_THREADS);           // [CP_THREADS]
    const int b = blockIdx.x, p0 = blockIdx.y * CP_PSLICE, tid = threadIdx.x;
    const float inv_r = 1.0f / (float)R;
    for (int c = tid; c < C; c += CP_THREADS) xbar[c] = 0.f;
    for (int k = 0; k < R; ++k) {
        const size_t m = (size_t)b * R + k;
        const int pos = cp_first_argmax(ids + m * L, L, sv, si);
        const hcp_bf16* tok = x + (m * L + pos) * C;
        float s = 0.f;
        for (int c = tid; c < C; c += CP_THREADS) s += hcp_bf2f(tok[c]);
        const float mean = cp_block_sum(s, red) / (float)C;
        float q = 0.f;
        for (int c = tid; c < C; c += CP_THREADS) { const float d = hcp_bf2f(tok[c]) - mean; q += d * d; }
        const float rstd = 1.0f / sqrtf(cp_block_sum(q, red) / (float)C + eps);
        for (int c = tid; c < C; c += CP_THREADS) xbar[c] += ((hcp_bf2f(tok[c]) - mean) * rstd * gamma[c] + beta[c]) * inv_r;
        if (blockIdx.y == 0 && tid == 0) { pos_out[m] = pos; stats[2 * m] = mean; stats[2 * m + 1] = rstd; }
    }
    HCP_SYNC();
    const int wave = tid >> 6, lane = tid & 63;
    for (int j = wave; j < CP_PSLICE && p0 + j < P; j += CP_THREADS / 64) {
        const int p = p0 + j;
        float acc = 0.f;
        for (int c = lane * 8; c < C; c += 64 * 8) {
            float w[8];
            cp_load_w8(W, w_f32, (size_t)p * C + c, w);
#pragma unroll
            for (int q = 0; q < 8; ++q) acc += w[q] * xbar[c + q];
        }
        acc = hcp_wave_sum(acc);
        if (lane == 0) pooled[(size_t)b * P + p] = acc;
    }
}

HCP_KERNEL(256) clip_pool_bwd_kernel(const hcp_bf16* x, const int* pos_in, const float* stats, const float* gamma, const void* W, int w_f32,
                                     const float* dpooled, hcp_bf16* dx, int R, int L, int C, int P) {
    HCP_DYN_SMEM(smem);
    float* g = (float*)smem;                     // [C] W^T d / r
    float* d = g + C;                            // [P] d_pooled[b] / r
    float* part = d + P;                         // [8][256] partial column sums over the 8 interleaved slices of P
    float* red = part + 8 * CP_THREADS;          // [4]
    const size_t m = blockIdx.x;
    const int b = (int)(m / R), tid = threadIdx.x;
    int pos = pos_in[m];
    pos = pos < 0 ? 0 : (pos >= L ? L - 1 : pos);             // (never write outside the row, whatever the buffer holds)
    const float inv_r = 1.0f / (float)R;
    for (int p = tid; p < P; p += CP_THREADS) d[p] = dpooled[(size_t)b * P + p] * inv_r;
    HCP_SYNC();
    const int cl = tid & 31, ps = tid >> 5;
    for (int c0 = 0; c0 < C; c0 += CP_THREADS) {
        const int c = c0 + cl * 8;
        float acc[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] = 0.f;
        if (c < C)
            for (int p = ps; p < P; p += 8) {
                float w[8];
                cp_load_w8(W, w_f32, (size_t)p * C + c, w);
                const float dp = d[p];
#pragma unroll
                for (int q = 0; q < 8; ++q) acc[q] += w[q] * dp;
            }
#pragma unroll
        for (int q = 0; q < 8; ++q) part[ps * CP_THREADS + cl * 8 + q] = acc[q];
        HCP_SYNC();
        if (c0 + tid < C) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) s += part[j * CP_THREADS + tid];
            g[c0 + tid] = s;
        }
        HCP_SYNC();
    }
    const float mean = stats[2 * m], rstd = stats[2 * m + 1];
    const hcp_bf16* tok = x + (m * L + pos) * C;
    float s1 = 0.f, s2 = 0.f;
    for (int c = tid; c < C; c += CP_THREADS) {
        const float dxn = g[c] * gamma[c], xh = (hcp_bf2f(tok[c]) - mean) * rstd;
        s1 += dxn; s2 += dxn * xh;
    }
    s1 = cp_block_sum(s1, red) / (float)C;
    s2 = cp_block_sum(s2, red) / (float)C;
    hcp_bf16* drow = dx + m * L * C;
    const int cv = C / 8;
    const long nv = (long)L * cv;
    for (long i = tid; i < nv; i += CP_THREADS)
        if ((int)(i / cv) != pos) *(hcp_bf16x8*)(drow + i * 8) = hcp_zero8();
    for (int c = tid; c < C; c += CP_THREADS) {
        const float dxn = g[c] * gamma[c], xh = (hcp_bf2f(tok[c]) - mean) * rstd;
        drow[(size_t)pos * C + c] = hcp_f2bf(rstd * (dxn - s1 - xh * s2));
    }
}

}  // namespace

HCP_API int hcp_clip_pool_fwd(const void* x, const long long* ids, const float* gamma, const float* beta, const void* W, int w_is_f32,
                              float* pooled, int* positions, float* stats, int B, int R, int L, int C, int P, float eps,
                              hipStream_t stream) {
    HCP_REQUIRE(x && ids && gamma && beta && W && pooled && positions && stats, "hcp_clip_pool_fwd: null pointer");
    HCP_REQUIRE(B > 0 && B < 65536 && R > 0 && L > 0 && C > 0 && C % 8 == 0 && C <= CP_MAX && P > 0 && P <= CP_MAX * CP_PSLICE && eps > 0.f,
                "hcp_clip_pool_fwd: bad shape (C %% 8 == 0, C <= %d)", CP_MAX);
    HCP_REQUIRE(((size_t)x | (size_t)W) % 16 == 0, "hcp_clip_pool_fwd: x and W must be 16-byte aligned");
    const size_t smem = (size_t)(C + 4) * sizeof(float) + CP_THREADS * (sizeof(long long) + sizeof(int));
    HCP_LAUNCH(clip_pool_fwd_kernel, dim3(B, hcp_cdiv(P, CP_PSLICE)), dim3(CP_THREADS), smem, stream, (const hcp_bf16*)x, ids, gamma, beta, W,
               w_is_f32, pooled, positions, stats, R, L, C, P, eps);
    HCP_LAUNCH_CHECK("clip_pool_fwd");
}

HCP_API int hcp_clip_pool_bwd(const void* x, const int* positions, const float* stats, const float* gamma, const void* W, int w_is_f32,
                              const float* d_pooled, void* dx, int B, int R, int L, int C, int P, hipStream_t stream) {
    HCP_REQUIRE(x && positions && stats && gamma && W && d_pooled && dx, "hcp_clip_pool_bwd: null pointer");
    HCP_REQUIRE(B > 0 && R > 0 && (long)B * R < 65536 && L > 0 && C > 0 && C % 8 == 0 && P > 0 && C + P <= CP_MAX,
                "hcp_clip_pool_bwd: bad shape (C %% 8 == 0, C + P <= %d)", CP_MAX);
    HCP_REQUIRE(((size_t)x | (size_t)W | (size_t)dx) % 16 == 0, "hcp_clip_pool_bwd: x, W and dx must be 16-byte aligned");
    const size_t smem = (size_t)(C + P + 8 * CP_THREADS + 4) * sizeof(float);
    HCP_LAUNCH(clip_pool_bwd_kernel, dim3(B * R), dim3(CP_THREADS), smem, stream, (const hcp_bf16*)x, positions, stats, gamma, W, w_is_f32,
               (const float*)d_pooled, (hcp_bf16*)dx, R, L, C, P);
    HCP_LAUNCH_CHECK("clip_pool_bwd");
}

HCP_API int hcp_embedding_pt_fwd_bf16(const long long* ids, int B, int R, int W, int n_word, const float* token_table, int vocab,
                                      const float* position_table, const long long* position_ids, int n_pos, const float* custom_table,
                                      int n_custom, const int* custom_map, int n_map, void* out, int* src_map, int C, hipStream_t stream) {
    HCP_REQUIRE(ids && token_table && position_table && out && src_map, "hcp_embedding_pt_fwd_bf16: null pointer");
    HCP_REQUIRE(B > 0 && R > 0 && W > 0 && n_word > 0 && vocab > 0 && n_pos > 0 && C > 0 && C % 8 == 0 && n_custom >= 0 && n_map >= 0,
                "hcp_embedding_pt_fwd_bf16: bad shape");
    HCP_REQUIRE(R * W <= PT_MAX_IDS && R * (n_word + 2) <= PT_MAX_IDS && R * W >= R * n_word + 1,
                "hcp_embedding_pt_fwd_bf16: need r*n_word + 1 <= r*w and r*w, r*(n_word + 2) <= %d", PT_MAX_IDS);
    HCP_REQUIRE(n_map == 0 || (custom_map && custom_table && n_custom > 0), "hcp_embedding_pt_fwd_bf16: custom words without a table");
    HCP_REQUIRE(((size_t)token_table | (size_t)position_table | (size_t)custom_table | (size_t)out) % 16 == 0,
                "hcp_embedding_pt_fwd_bf16: tables and output must be 16-byte aligned");
    const size_t smem = (size_t)(4 * PT_MAX_IDS + 2 * PT_THREADS) * sizeof(int);
    HCP_LAUNCH(embedding_pt_fwd_kernel, dim3(B), dim3(PT_THREADS), smem, stream, ids, R, W, n_word, token_table, vocab, position_table,
               position_ids, n_pos, custom_table, n_custom, custom_map, n_map, (hcp_bf16*)out, src_map, C);
    HCP_LAUNCH_CHECK("embedding_pt_fwd_bf16");
}

HCP_API int hcp_embedding_pt_bwd_f32(const void* dx, const int* src_map, long M, int C, float* grad, int n_custom, int beta,
                                     hipStream_t stream) {
    HCP_REQUIRE(dx && src_map && grad, "hcp_embedding_pt_bwd_f32: null pointer");
    HCP_REQUIRE(M > 0 && C > 0 && n_custom > 0 && (beta == 0 || beta == 1), "hcp_embedding_pt_bwd_f32: bad shape");
    const size_t smem = (size_t)PT_BWD_CHUNK * sizeof(int);
    HCP_LAUNCH(embedding_pt_bwd_kernel, dim3(n_custom, hcp_cdiv(C, PT_THREADS)), dim3(PT_THREADS), smem, stream, (const hcp_bf16*)dx,
               src_map, M, C, grad, beta);
    HCP_LAUNCH_CHECK("embedding_pt_bwd_f32");
}
