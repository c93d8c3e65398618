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

}  // namespace

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
