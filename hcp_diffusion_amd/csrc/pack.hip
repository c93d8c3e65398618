// pack.hip — refresh of the bf16 operand copies of trainable host weights after an optimizer step (full fine-tuning).
//
// The fp32 masters live in one flat bucket (fullft.HostBucket); the GEMM / conv kernels read bf16 operands in two
// layouts per layer: row-major [N][K] (forward) and its transpose [K][N] (data gradient) — for 3x3 convolutions per
// tap: [Cout][tap][Cin] and [Cin][tap][Cout].  ONE grouped launch converts and transposes every layer: a workgroup
// looks its 64x64 tile up in a prefix table of 2-D pieces (a Linear is one piece, a 3x3 conv nine).  HBM-bound:
// 4 B read + 2 x 2 B written per parameter (SD1.5: 6.9 GB per step).  The conv (LoCon) LoRA factors use the same launch to
// build their operand images (W_down per tap -> [32][tap][Cin] and [Cin][tap][32]; alpha * W_up -> [Cout][32] and [32][Cout]).
#include "hcp_common.h"

namespace {

struct PackPiece {              // 56 bytes, mirrored by fullft.py (numpy structured dtype)
    const float* src;           // fp32 [rows][src_ld]
    hcp_bf16* dst_rm;           // bf16 [rows][rm_ld]   (may be null)
    hcp_bf16* dst_tr;           // bf16 [cols][tr_ld]   (may be null)
    int rows, cols, src_ld, rm_ld, tr_ld;
    int tile0;                  // index of this piece's first tile in the launch
    int tiles_c;                // tiles along the column dimension
    float scale;                // multiplies every element (LoRA: alpha folded into the W_up operand); 1.0 for plain copies
};
static_assert(sizeof(PackPiece) == 56, "descriptor layout is part of the ABI");

HCP_KERNEL(256) pack_weights_kernel(const PackPiece* pieces, int count) {
    HCP_DYN_SMEM(smem);
    hcp_bf16* tile = (hcp_bf16*)smem;                       // [64][66]
    constexpr int TS = 66;
    int lo = 0, hi = count - 1;                             // last piece with tile0 <= blockIdx.x
    const int b = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pieces[mid].tile0 <= b) lo = mid; else hi = mid - 1;
    }
    const PackPiece pc = pieces[lo];
    const int t = b - pc.tile0;
    const int r0 = (t / pc.tiles_c) * 64, c0 = (t % pc.tiles_c) * 64;
    const int tid = threadIdx.x;
    const int cc = tid & 63, rg = tid >> 6;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
        const int rr = rg + 4 * i;
        const int r = r0 + rr, c = c0 + cc;
        hcp_bf16 v = 0;
        if (r < pc.rows && c < pc.cols) {
            v = hcp_f2bf(pc.src[(size_t)r * pc.src_ld + c] * pc.scale);
            if (pc.dst_rm) pc.dst_rm[(size_t)r * pc.rm_ld + c] = v;
        }
        tile[rr * TS + cc] = v;
    }
    if (!pc.dst_tr) return;                                 // block-uniform
    HCP_SYNC();
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
        const int ci = rg + 4 * i;                          // transposed row = source column
        const int c = c0 + ci, r = r0 + cc;
        if (c < pc.cols && r < pc.rows) pc.dst_tr[(size_t)c * pc.tr_ld + r] = tile[cc * TS + ci];
    }
}

// Folded images of an upsampler's 3x3 weight (include/hcp_mi355x.h: hcp_conv_fold_pack).  Behind a nearest-2x upsample the kernel rows
// that read the same source row add up: output parity 0 reads source row y - 1 through ky = 0 and row y through ky = 1, 2; parity 1 reads
// row y through ky = 0, 1 and row y + 1 through ky = 2 (columns alike).  The taps are summed in fp32 in ascending (ky, kx) order and rounded
// to bf16 ONCE.  One thread per output element, a one-off per frozen weight (the transposed image reads W with stride 9 Cin: not tuned).
//   forward image  Wf  [py][px][Cout][ty][tx][Cin]: ky in {0} | {1, 2} (py = 0), {0, 1} | {2} (py = 1) for ty = 0 | 1
//   data gradient  Wdf [Cin][ay][ax][Cout_pad]:     ky in {2}, {1, 2}, {0, 1}, {0} for ay = 0 .. 3 (dY row 2 y + ay - 1); Cout_pad = Cout
//                  rounded up to whole 64-channel K tiles, zeros in the padding
HCP_DEVICE float fold_sum(const float* w, int klo_y, int khi_y, int klo_x, int khi_x, int cin) {
    float sacc = 0.f;
    bool first = true;
    for (int ky = klo_y; ky <= khi_y; ++ky)
        for (int kx = klo_x; kx <= khi_x; ++kx) {
            const float v = w[(size_t)(ky * 3 + kx) * cin];
            sacc = first ? v : sacc + v;
            first = false;
        }
    return sacc;
}
HCP_KERNEL(256) conv_fold_pack_kernel(const float* W, hcp_bf16* Wf, hcp_bf16* Wdf, int Cout, int Cin) {
    const long n = (long)16 * Cout * Cin;
    const int Cp = (Cout + 63) / 64 * 64;
    const long nd = (long)16 * Cp * Cin;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n + nd; idx += (long)gridDim.x * 256) {
        if (idx < n) {                                      // forward image: idx = ((((py 2 + px) Cout + co) 2 + ty) 2 + tx) Cin + ci
            const int ci = (int)(idx % Cin); long r = idx / Cin;
            const int tx = (int)(r & 1), ty = (int)((r >> 1) & 1); r >>= 2;
            const int co = (int)(r % Cout), q = (int)(r / Cout), py = q >> 1, px = q & 1;
            const int ylo = py == 0 ? (ty == 0 ? 0 : 1) : (ty == 0 ? 0 : 2), yhi = py == 0 ? (ty == 0 ? 0 : 2) : (ty == 0 ? 1 : 2);
            const int xlo = px == 0 ? (tx == 0 ? 0 : 1) : (tx == 0 ? 0 : 2), xhi = px == 0 ? (tx == 0 ? 0 : 2) : (tx == 0 ? 1 : 2);
            Wf[idx] = hcp_f2bf(fold_sum(W + (size_t)co * 9 * Cin + ci, ylo, yhi, xlo, xhi, Cin));
        } else {                                            // data-gradient image: j = ((ci 4 + ay) 4 + ax) Cout_pad + co
            const long j = idx - n;
            const int co = (int)(j % Cp); long r = j / Cp;
            if (co >= Cout) { Wdf[j] = 0; continue; }
            const int ax = (int)(r & 3), ay = (int)((r >> 2) & 3); const int ci = (int)(r >> 4);
            const int ylo = ay == 0 ? 2 : (ay == 1 ? 1 : 0), yhi = ay == 0 ? 2 : (ay == 1 ? 2 : (ay == 2 ? 1 : 0));
            const int xlo = ax == 0 ? 2 : (ax == 1 ? 1 : 0), xhi = ax == 0 ? 2 : (ax == 1 ? 2 : (ax == 2 ? 1 : 0));
            Wdf[j] = hcp_f2bf(fold_sum(W + (size_t)co * 9 * Cin + ci, ylo, yhi, xlo, xhi, Cin));
        }
    }
}

}  // namespace

HCP_API int hcp_conv_fold_pack(const float* W, void* Wf, void* Wdf, int Cout, int Cin, hipStream_t stream) {
    HCP_REQUIRE(W && Wf && Wdf && Cout > 0 && Cin > 0, "hcp_conv_fold_pack: bad arguments");
    const long n = (long)16 * Cin * (Cout + (Cout + 63) / 64 * 64);
    int g = (int)((n + 255) / 256); if (g > 8192) g = 8192;
    HCP_LAUNCH(conv_fold_pack_kernel, dim3(g), dim3(256), 0, stream, W, (hcp_bf16*)Wf, (hcp_bf16*)Wdf, Cout, Cin);
    HCP_LAUNCH_CHECK("conv_fold_pack");
}

HCP_API int hcp_pack_piece_bytes(void) { return (int)sizeof(PackPiece); }

// pieces: device array of `count` PackPiece descriptors sorted by tile0; total_tiles = sum of their 64x64 tiles.
HCP_API int hcp_pack_weights(const void* pieces, int count, int total_tiles, hipStream_t stream) {
    HCP_REQUIRE(pieces && count > 0 && total_tiles > 0, "hcp_pack_weights: bad arguments");
    HCP_LAUNCH(pack_weights_kernel, dim3(total_tiles), dim3(256), 64 * 66 * sizeof(hcp_bf16), stream, (const PackPiece*)pieces, count);
    HCP_LAUNCH_CHECK("pack_weights");
}
