/* hcp_mi355x.h — C ABI of libhcp_mi355x.so: the MI355X (gfx950) kernels behind HCP-Diffusion's fine-tuning hot path.
 *
 * The reference (IrisRainbowNeko/HCP-Diffusion v0.9.1) is pure Python; its hot path
 *   Trainer.train_one_step            hcpdiff/train_ac.py:467-504
 *   -> TEUnetWrapper.forward          hcpdiff/models/wrapper.py:14-30   (self.unet(...).sample, :29)
 *   -> LoraPatchContainer.forward     hcpdiff/models/lora_base_patch.py:20-35
 * bottoms out in torch / diffusers ops.  Each entry point below replaces one of those ops; the comment on each
 * names the reference call it stands in for.  Binding a maintainer would add: ctypes, see INTEGRATION.md.
 *
 * Conventions: every function returns 0 on success, <0 on error (message: hcp_last_error(), thread-local);
 * raw DEVICE pointers, explicit shapes/strides (in elements), a hipStream_t; no allocation (workspace sizes are
 * queryable), no stream synchronisation, re-entrant, callable from any thread (autograd runs backward on its own).
 * bf16 tensors are raw uint16 bit patterns; "NHWC" = channels-last [B,H,W,C] == token-major [B,H*W,C].
 */
#ifndef HCP_MI355X_H
#define HCP_MI355X_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hcpStream_t; /* == hipStream_t */

const char* hcp_last_error(void);
int hcp_is_emulated(void); /* 0 for the product library */
/* Revision of this header.  hcp_abi_version() returns the value the library was built with; a binding made for another revision must
 * refuse to call it (hcp_diffusion_amd/_lib.py does).  1: rounds 1-5.  2: round 6 — workspace arguments on the LoRA weight-gradient
 * entry points (slabs + ordered reduce instead of fp32 atomics), 152-byte grouped descriptors; earlier in-place argument insertions
 * (ldt on hcp_gemm_lora_bf16 / hcp_gemm_geglu_bwd_bf16, l_lo, ldu / ldt) are covered by the same bump.  3: round 6 — the (hi | lo)
 * residual stream: residual_lo / D_lo on hcp_gemm_bf16 / hcp_gemm_lora_bf16, x_lo / addend_lo / dx_lo on hcp_layernorm_fwd / _bwd; the
 * GEGLU-forward output gact on hcp_gemm_bf16 / hcp_gemm_lora_bf16.  4: prompt tuning — hcp_embedding_pt_fwd_bf16 /
 * hcp_embedding_pt_bwd_f32 (csrc/embedding.hip).  5: folded upsampler convs — hcp_conv_fold_pack / hcp_conv3x3_up_fold_bf16.
 * 6: SDXL's second text encoder — hcp_gelu, hcp_clip_pool_fwd / hcp_clip_pool_bwd.  7: pyramid noise — hcp_pyramid_noise_accum /
 * hcp_pyramid_noise_finish (csrc/noise.hip).  8: native LoRA dropout — hcp_dropout_residual_fwd / hcp_dropout_bwd /
 * hcp_dropout_advance (csrc/dropout.hip).  9: Euler / Euler-ancestral sampler — hcp_euler_step / hcp_sampler_advance /
 * hcp_sampler_begin (csrc/sampler.hip). */
#define HCP_ABI_VERSION 9
int hcp_abi_version(void);
/* Device self-check of the fp32 atomic path (no reference counterpart: the reference's sums are torch's).  workgroups x 256 threads add
 * small integers into line[16] and into bucket[i * stride], i < nb (both cleared here first); exact expected values:
 * line[j] = workgroups * 16 * ((j & 3) + 1), bucket[i * stride] = sum of ((t & 3) + 1) over (w, t) with (37 w + 101 t) % nb == i. */
int hcp_selfcheck_atomics(float* line, float* bucket, int nb, int stride, int workgroups, hcpStream_t stream);

/* D[M,N] = alpha*(A[M,K] B[N,K]^T + A2[M,K2] B2[N,K2]^T) + bias[N] + rowbias[m/rows_per_group, :] + residual[M,N]
 * Replaces nn.Linear / 1x1 nn.Conv2d forward and input-gradient of the UNet, and the LoRA container's
 * torch.mm(x, (W_host + alpha*W_up@W_down)^T) + bias (lora_layers_patch.py:50-57, lora_base_patch.py:68-74):
 * (A2,B2) is the rank-r side path (x W_down^T, alpha*W_up) appended to the reduction. */
int hcp_gemm_bf16(const void* A, int lda, const void* B, int ldb, void* D, int ldd, int M, int N, int K, const void* A2,
                  int lda2, const void* B2, int ldb2, int K2, const float* bias, const float* rowbias, int rowbias_ld,
                  int rows_per_group, const void* residual, int ldr, const void* residual_lo, void* D_lo, void* gact, float alpha,
                  int out_f32, void* workspace, size_t workspace_bytes, hcpStream_t stream);
/* (hi | lo) residual stream, ABI 3: residual_lo / D_lo (both optional, bf16, leading dimensions ldr / ldd).  A transformer block's
 * residual stream x is carried as hi = bf16(x) and lo = bf16(x - hi): the epilogue adds residual + residual_lo in fp32 and writes
 * D = bf16(v), D_lo = bf16(v - D) — the 16 mantissa bits the reference's LoRA layers keep on that stream by returning
 * mm(x, W^T) [bf16 under autocast] + bias [fp32] = fp32 (lora_layers_patch.py:50-57).  NULL, NULL = the plain bf16 epilogue.
 * GEGLU forward, ABI 3: gact (optional, bf16 [M, N/2]).  D = (h | g) is the output of diffusers' GEGLU projection (FeedForward.net[0].proj,
 * cfgs/unet_struct.txt:27-30): gact = bf16(h * gelu(g)) is formed in the same epilogue from the fp32 values (the stand-alone hcp_geglu_fwd
 * pass and one rounding disappear: the reference's LoRA layer hands GEGLU an fp32 (h | g) too).  Needs a contiguous bf16 D (ldd = N),
 * N % 16 == 0, no residual / row bias / alpha; where the dispatched tile cannot pair the halves the library runs hcp_geglu_fwd itself. */
/* Fused LoRA linear, forward and input-gradient: T = A L^T (rank slot 32, written to Tout if non-NULL),
 * D = A B^T + T E^T + bias + residual in ONE launch (the block accumulates its T tile from the A tiles it streams);
 * deep-K / small-M shapes run as two launches (T GEMM, then split-K K-extension GEMM) and then require Tout.
 * ldt = 32: T is rounded to bf16 (Tout [M,32]).  ldt = 64: "split" T — the fp32 accumulator leaves as T_hi = bf16(T) and
 * T_lo = bf16(T - T_hi), the product takes both (D += T_hi E^T + T_lo E^T) and Tout [M,64] = (T_hi | T_lo) for hcp_lora_wgrad*:
 * the rank-r intermediate keeps 16 mantissa bits, as the reference's merged-weight form never rounds it at all
 * (the two-launch form keeps the rounded T and zeroes the residual half).
 * Replaces LoraPatchContainer.forward's weight merge + mm (lora_base_patch.py:20-35,61-74). */
int hcp_gemm_lora_bf16(const void* A, int lda, const void* B, int ldb, const void* L, const void* E, void* Tout, int ldt, void* D,
                       int ldd, int M, int N, int K, const float* bias, const void* residual, int ldr, const void* residual_lo, void* D_lo,
                       void* gact, void* workspace, size_t workspace_bytes, hcpStream_t stream);
/* FF-out input-gradient with the GEGLU backward in its epilogue: dY_ff = A B^T (+ the LoRA side path as hcp_gemm_lora_bf16's backward
 * form: L = W_up^T, E = alpha W_down^T, Tout = dY W_up; L = E = NULL for a plain host) is never written; with (h | g) = HG[M, 2F] saved
 * by the forward, DHG[m, n] = dY_ff gelu(g), DHG[m, F + n] = dY_ff h gelu'(g).  Replaces the dX GEMM of FeedForward.net[2] + the
 * GEGLU backward pass (diffusers GEGLU in BasicTransformerBlock.ff, reference cfgs/unet_struct.txt:27-33 / autograd of F.gelu). */
int hcp_gemm_geglu_bwd_bf16(const void* A, int lda, const void* B, int ldb, const void* L, const void* E, void* Tout, int ldt,
                            const void* HG, void* DHG, int M, int F, int K, void* workspace, size_t workspace_bytes, hcpStream_t stream);
/* fp32 split-K scratch (optional: workspace may be NULL, then small-M problems run unsplit). */
size_t hcp_gemm_workspace_bytes(int M, int N);

/* 3x3 convolution over NHWC bf16 as an implicit GEMM.  mode 0: forward, Wp = [Cout][3][3][C1+C2];
 * mode 1: data gradient, X1 = dY, Wp = [Cin][3][3][Cout].  pad 1 = padding 1 (every conv of the UNet); pad 0 (forward only) = taps
 * 0..+2 with zeros past the bottom/right edge, i.e. F.pad(x,(0,1,0,1)) + padding 0: the VAE encoder's Downsample2D.
 * Options: stride 1|2, nearest-2x upsampled source,
 * second source tensor (channel concat), bias, per-sample row bias (time embedding), residual, and a rank-32 K-extension
 * D += A2[M,32] B2[Cout,32]^T — the conv (LoCon) LoRA side path T (alpha W_up)^T, T = conv3x3(x, W_down)
 * (reference lora_layers_patch.py:64-100 merges W + alpha * einsum(W_up, W_down) into the conv weight instead).
 * Replaces F.conv2d in diffusers ResnetBlock2D / Downsample2D / Upsample2D (reference cfgs/unet_struct.txt:92-114,390-393). */
int hcp_conv3x3_bf16(const void* X1, int C1, const void* X2, int C2, int B, int Hs, int Ws, int Ho, int Wo, int mode,
                     int stride, int upsample, int pad, const void* Wp, int Cout, void* D, int ldd, const float* bias,
                     const float* rowbias, int rowbias_ld, const void* residual, int ldr, int out_f32, const void* A2,
                     const void* B2, void* workspace, size_t workspace_bytes, hcpStream_t stream);
/* The 3x3 / pad-1 convolution behind a nearest-2x upsample (diffusers Upsample2D = F.interpolate(x, 2.0, "nearest") + conv) with FOLDED
 * weights: every 2x2 block of the upsampled image is one source pixel, so the nine taps collapse to 2x2 per output parity (4/9 of the
 * multiply-adds).  hcp_conv_fold_pack builds both images from the fp32 master W [Cout][3][3][Cin] (taps summed in fp32, one rounding):
 *   Wf  [py][px][Cout][2][2][Cin]: rows (ky) {0} | {1,2} for py = 0, {0,1} | {2} for py = 1; columns alike
 *   Wdf [Cin][4][4][Cout_pad]: taps {2}, {1,2}, {0,1}, {0} per axis — one 4x4 stride-2 pad-1 convolution over the high-resolution dY;
 *       Cout_pad = Cout rounded up to a multiple of 64, zeros in the padding
 * hcp_conv3x3_up_fold_bf16 (Hs x Ws = the LOW resolution; Cin % 64 == 0, Cout % 160 == 0):
 *   mode 0: X [B,Hs,Ws,Cin], Wfold = Wf -> D [B,2Hs,2Ws,Cout] (+ bias);  mode 1: X = dY [B,2Hs,2Ws,Cout], Wfold = Wdf -> D = dX [B,Hs,Ws,Cin].
 * For frozen weights only (the images are built once); returns 1 without launching only under the tools switch hcp_debug_set_conv_fold(0). */
int hcp_conv_fold_pack(const float* W, void* Wf, void* Wdf, int Cout, int Cin, hcpStream_t stream);
int hcp_conv3x3_up_fold_bf16(const void* X, int B, int Hs, int Ws, int Cin, int Cout, int mode, const void* Wfold, void* D,
                             const float* bias, void* workspace, size_t workspace_bytes, hcpStream_t stream);

/* Fused attention, element (b,n,h,c) at base + b*bs + n*rs + h*D + c; lse[B,H,Nq] = logsumexp(scale*QK^T).
 * Replaces diffusers CrossAttention/AttnProcessor2_0 (SDPA) or xformers (reference train_ac.py:258-260). D in {40,64,80,160}. */
/* key_bias (optional, fp32 [B,Nk], batch stride key_bias_bs): additive bias on the SCALED scores of every head/query —
 * diffusers' encoder_attention_mask -> (1 - mask) * -10000 (the attn_mask the reference passes at models/wrapper.py:22-29).
 * `causal` is a flag word.  bit 0 (self-attention only, Nq == Nk): key k contributes to query q only if k <= q — the CLIP text encoder's
 * causal_attention_mask (cfgs/te_struct.txt CLIPAttention; text-encoder LoRA, cfgs/train/examples/lora_conventional.yaml:14-19). 
 * bit 1 (unmasked problems only): Q already holds Q * scale * log2(e) — the caller folded the factor into the weights of the Q
 * projection (and into the LoRA alpha of that layer), so the score accumulator is the exp2 argument and no multiply precedes the
 * exponential; `scale` still names the softmax scale.  hcp_attention_bwd then returns dQ as the gradient w.r.t. THAT tensor. */
int hcp_attention_fwd(const void* Q, const void* K, const void* V, void* O, float* lse, int B, int H, int Nq, int Nk, int D,
                      long q_bs, int q_rs, long k_bs, int k_rs, long v_bs, int v_rs, long o_bs, int o_rs, float scale,
                      const float* key_bias, long key_bias_bs, int causal, hcpStream_t stream);
/* workspace (optional, 2*B*Nk*H*D floats): lets short-key problems split the dK/dV query loop across workgroups */
int hcp_attention_bwd(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* lse,
                      float* delta_ws /* [B,H,Nq] */, void* dQ, void* dK, void* dV, int B, int H, int Nq, int Nk, int D,
                      long q_bs, int q_rs, long k_bs, int k_rs, long v_bs, int v_rs, long o_bs, int o_rs, float scale,
                      const float* key_bias, long key_bias_bs, int causal, void* workspace, size_t workspace_bytes,
                      hcpStream_t stream);


/* GroupNorm (+SiLU) over NHWC; stats[B,G,2] = (mean, rstd).  Replaces F.group_norm + SiLU
 * (unet_struct.txt:13,93,97,929).  Backward returns dx only (affine parameters frozen). */
size_t hcp_groupnorm_workspace_bytes(int B, int HW, int C, int G);
int hcp_groupnorm_silu_fwd(const void* x, const float* gamma, const float* beta, void* y, float* stats, void* workspace,
                           int B, int HW, int C, int G, float eps, int silu, hcpStream_t stream);
int hcp_groupnorm_silu_bwd(const void* x, const void* dy, const float* gamma, const float* beta, const float* stats,
                           const void* addend /* optional residual-path gradient, added in the same pass */, void* dx,
                           void* workspace, int B, int HW, int C, int G, int silu, hcpStream_t stream);

/* LayerNorm over the last dim; stats[M,2] = (mean, rstd).  Replaces F.layer_norm (unet_struct.txt:44-46).
 * x_lo / addend_lo / dx_lo (optional, ABI 3): the lo images of a (hi | lo) residual stream (see hcp_gemm_bf16) — the row normalised is
 * x + x_lo, the gradient arriving on the residual path is addend + addend_lo, and the result leaves as dx = bf16(g), dx_lo = bf16(g - dx). */
int hcp_layernorm_fwd(const void* x, const void* x_lo, const float* gamma, const float* beta, void* y, float* stats, int M, int C,
                      float eps, hcpStream_t stream);
int hcp_layernorm_bwd(const void* x, const void* x_lo, const void* dy, const float* gamma, const float* stats, const void* addend,
                      const void* addend_lo, void* dx, void* dx_lo, int M, int C, hcpStream_t stream);

/* y[M,F] = h[:, :F] * gelu(h[:, F:])   (diffusers GEGLU, unet_struct.txt:28-30) */
int hcp_geglu_fwd(const void* h, void* y, long M, int F, hcpStream_t stream);
int hcp_geglu_bwd(const void* h, const void* dy, void* dh, long M, int F, hcpStream_t stream);

int hcp_add_bf16(const void* a, const void* b, void* out, long n, hcpStream_t stream);
/* LoRA layer-output dropout (lora_base_patch.py:74) with a counter-based mask that is never stored (csrc/dropout.hip).  state: device
 * int64[2] = (seed, calls).  A group is 8 consecutive bf16 elements; group g draws Philox4x32-10 with counter (lo32, hi32 of group_base + g,
 * layer_id, lo32(calls)) and key (lo32, hi32 of seed); element 8g + 2j takes the low 16 bits of output word j, 8g + 2j + 1 the high 16.
 * keep iff that value >= T = round(p * 65536); survivors are scaled by 1 / (1 - T / 65536) (p >= 1: zeros).
 * fwd: out = bf16(keep ? y * scale : 0 (+ residual)), fp32 arithmetic, one rounding; residual may be NULL; out may alias y.
 * bwd: dx = keep ? dy * scale : 0 (the residual's gradient is dy itself); dx may alias dy.  n % 8 == 0, 16-byte aligned buffers.
 * advance: state[1] += 1 (one launch per training forward of a module, before any of its layers runs). */
int hcp_dropout_residual_fwd(const void* y, const void* residual, void* out, long n, const long long* state, unsigned layer_id,
                             unsigned long long group_base, double p, hcpStream_t stream);
int hcp_dropout_bwd(const void* dy, void* dx, long n, const long long* state, unsigned layer_id, unsigned long long group_base, double p,
                    hcpStream_t stream);
int hcp_dropout_advance(long long* state, hcpStream_t stream);
int hcp_copy2d_bf16(const void* src, int sld, void* dst, int dld, long M, int C, hcpStream_t stream); /* skip concat/split */
/* torch.cat([h, skip], dim=1) of the up-block ResnetBlock2D and its gradient split in one launch: joint [M][c1+c2] <-> a [M][c1], b [M][c2];
 * split = 0 writes joint, split = 1 writes a and b (c1, c2 multiples of 8). */
int hcp_concat2_bf16(void* a, int c1, void* b, int c2, void* joint, long M, int split, hcpStream_t stream);
int hcp_silu_fwd(const void* x, void* y, long n, hcpStream_t stream);
int hcp_silu_bwd(const void* x, const void* dy, void* dx, long n, hcpStream_t stream);
int hcp_nchw_to_nhwc_bf16(const void* src, int src_is_f32, void* dst, int B, int C, int HW, int Cpad, hcpStream_t stream);
int hcp_nhwc_to_nchw_f32(const float* src, float* dst, int B, int C, int HW, int Csrc, hcpStream_t stream);
int hcp_upsample2x_bwd(const void* dup, void* dx, int B, int H, int W, int C, hcpStream_t stream);

/* ---- host-layer weight gradients (full fine-tuning: cfgs/train/examples/DreamBooth.yaml:6-10 trains every UNet
 * parameter; autograd's dW of nn.Linear / nn.Conv2d [ext]).  fp32 `+=` into the gradient buffer: token-split partial sums go to
 * workspace slabs that a reduce kernel adds in split order (no atomics, bit-reproducible); only hcp_colsum_bf16 adds with fp32
 * atomics. ---- */
/* dW[N,K] += dY[M,N]^T X[M,K]; workspace = optional fp32 scratch for token-split partial sums */
int hcp_wgrad_linear_bf16(const void* dY, int ldy, const void* X, int ldx, float* dW, int ldw, int M, int N, int K,
                          float* workspace, size_t workspace_bytes, hcpStream_t stream);
/* dW[Cout][3][3][Cw] += dY^T im2col(X1|X2): same gather as hcp_conv3x3_bf16 (stride, nearest-2x upsample, concat);
 * layout = torch channels_last storage of the diffusers weight [Cout,Cin,3,3] */
int hcp_wgrad_conv3x3_bf16(const void* dY, int ldy, const void* X1, int C1, const void* X2, int C2, float* dW, int Cw, int B,
                           int Hs, int Ws, int Ho, int Wo, int Cout, int stride, int upsample, float* workspace,
                           size_t workspace_bytes, hcpStream_t stream);
/* out[g][n] += sum of rows of group g of Y (bias gradients; per-sample time-embedding row-bias gradient) */
int hcp_colsum_bf16(const void* Y, int ldy, float* out, int ldo, int M, int N, int rows_per_group, hcpStream_t stream);
/* After the optimizer step of a full fine-tune: refresh every layer's bf16 operand copies (row-major + transposed) from
 * the fp32 masters in ONE grouped launch.  pieces = device array of 56-byte descriptors
 * {const float* src; bf16* dst_rm; bf16* dst_tr; int rows, cols, src_ld, rm_ld, tr_ld, tile0, tiles_c; float scale;} sorted by tile0. */
int hcp_pack_piece_bytes(void);
int hcp_pack_weights(const void* pieces, int count, int total_tiles, hcpStream_t stream);
/* norm weight / bias gradients: dgamma[c] += sum dz * xhat, dbeta[c] += sum dz (dz includes the fused SiLU'), stats
 * as saved by the forward entry points */
int hcp_groupnorm_affine_grad(const void* x, const void* dy, const float* gamma, const float* beta, const float* stats,
                              float* dgamma, float* dbeta, int B, int HW, int C, int G, int silu, hcpStream_t stream);
int hcp_layernorm_affine_grad(const void* x, const void* dy, const float* stats, float* dgamma, float* dbeta, int M, int C,
                              hcpStream_t stream);

/* Timesteps(flip_sin_to_cos=True, freq_shift=0) (unet_struct.txt:3): emb[b] = [cos(t f_i) | sin(t f_i)] */
int hcp_timestep_embedding(const long long* timesteps, void* emb, int B, int dim, float max_period, hcpStream_t stream);
/* same for fp32 inputs: SDXL's add_time_proj over added_cond_kwargs["time_ids"] (= crop_info, models/wrapper.py:66) */
int hcp_timestep_embedding_f32(const float* values, void* emb, int B, int dim, float max_period, hcpStream_t stream);
/* DDPMScheduler.add_noise as called by train_ac.py:447 */
int hcp_add_noise(const float* x0, const float* noise, const long long* timesteps, const float* alphas_cumprod, float* xt,
                  int B, long per_sample, hcpStream_t stream);
/* Pyramid (multi-resolution) noise, PyramidNoiseScheduler.add_noise (reference hcpdiff/noise/pyramid_noise.py:17-32), as two launches
 * whatever the number of levels (csrc/noise.hip).
 * hcp_pyramid_noise_accum: noise fp32 [B, C, h, w], IN PLACE: noise += resize(field_i -> (h, w)) * discount^i for i = 1 .. *n_active.
 * fields: HOST array of n_max (<= HCP_PYRAMID_MAX_LEVELS) device pointers, field_elems: HOST array of the floats each buffer holds;
 * level i is read as a contiguous [B, C, hn_i, wn_i] tensor at the start of its buffer, which may be larger.  dims: DEVICE int32
 * [n_max][2] = (hn_i, wn_i) and n_active: DEVICE int32 — one captured graph serves every draw of the sizes; a table the buffers cannot
 * serve (a size < 1, B C hn wn above field_elems[i], *n_active outside [0, n_max]) reads nothing and leaves NaN in noise.  mode 0:
 * bilinear as F.interpolate(align_corners=False) — src = max((dst + 0.5) in/out - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, in - 1);
 * mode 1: nearest, floor(dst in/out); any other mode is refused.  partials: 2 * HCP_PYRAMID_PARTIALS doubles of workspace: every
 * workgroup leaves the sum and the sum of squares of its results (double, fixed order, no atomics: the same bits on every run).
 * hcp_pyramid_noise_finish (same B, C, h, w): adds the partials in index order to std = the unbiased (N - 1) standard deviation over
 * the whole tensor, as Tensor.std(), and writes xt = sqrt(acp[t_b]) x0 + sqrt(1 - acp[t_b]) noise / std.  noise stays the UNNORMALISED
 * sum: the reference adds into the caller's tensor in place (:28) and normalises a new one (:31), so its loss target is the sum.
 * std_out: null, or one device float that receives std. */
#define HCP_PYRAMID_MAX_LEVELS 16
#define HCP_PYRAMID_PARTIALS 4096
int hcp_pyramid_noise_accum(float* noise, const float* const* fields, const long* field_elems, int n_max, const int* dims,
                            const int* n_active, double discount, int mode, double* partials, int B, int C, int h, int w,
                            hcpStream_t stream);
int hcp_pyramid_noise_finish(const float* x0, const float* noise, const long long* timesteps, const float* alphas_cumprod, float* xt,
                             const double* partials, float* std_out, int B, int C, int h, int w, hcpStream_t stream);
/* --- VAE encode (AutoencoderKL.encode(...).latent_dist.sample() * scaling_factor, reference
 * data/pair_dataset.py:72-75 and train_ac.py:428-435).  The encoder reuses the conv / GroupNorm / GEMM entry points above; these
 * three finish it: the single-head d=512 mid-block attention runs as GEMM -> hcp_softmax_rows -> GEMM (V transposed by
 * hcp_transpose_bf16), and hcp_vae_latent_sample folds quant_conv (1x1), the logvar clamp [-30,20] and the reparameterised
 * draw (noise == NULL: the mode) into one pass over the fp32 moments [B,2L,hw]. */
int hcp_transpose_bf16(const void* src, void* dst, int batch, int R, int C, hcpStream_t stream);
int hcp_softmax_rows(const float* S, long lds, void* P, long ldp, int M, int N, float scale, hcpStream_t stream);
int hcp_vae_latent_sample(const float* moments, const float* Wq, const float* bq, const float* noise, float* latents, int B, int L,
                          long hw, float scale, hcpStream_t stream);
/* --- text encoder (CLIP, cfgs/te_struct.txt; text-encoder LoRA of cfgs/train/examples/lora_conventional.yaml:14-19): its linears,
 * LayerNorms and (causal) attention are the entry points above; these two are its embedding lookup and MLP activation. */
int hcp_quick_gelu(const void* x, const void* dy, void* out, long n, hcpStream_t stream);   /* dy NULL: forward; else dx */
int hcp_embedding_bf16(const float* token_table, const long long* ids, const float* position_table, const long long* position_ids,
                       void* out, long n, int C, int L, hcpStream_t stream);
/* Prompt tuning (EmbeddingPTHook, hcpdiff/models/text_emb_ex.py:33-69, then CLIPTextEmbeddings' position add; csrc/embedding.hip).
 * ids [B, R*W] int64 (the hook's regrouped layout); custom_map int32 [n_map][2] = (row offset into custom_table [n_custom, C], n_vec)
 * of token id vocab + i.  Per batch item each id >= vocab with a registered word becomes its n_vec custom rows, rows [1, R*n_word + 1)
 * of the expanded sequence are cut into R chunks of n_word, and every chunk gets BOS / EOS = token rows of ids[0][0] / ids[0][R*W-1]
 * (batch item 0, ids clipped to [0, vocab-1]).  out bf16 [B*R, n_word+2, C] = bf16(src_row + position_table[position_ids or j]) in fp32;
 * src_map int32 [B*R, n_word+2]: >= 0 token row, < 0 custom row -1 - code.  Unregistered ids >= vocab (and negative ids) read the
 * clipped token row.  Needs R*n_word + 1 <= R*W <= 2048, R*(n_word+2) <= 2048, C % 8 == 0, 16-byte aligned tables. */
int hcp_embedding_pt_fwd_bf16(const long long* ids, int B, int R, int W, int n_word, const float* token_table, int vocab,
                              const float* position_table, const long long* position_ids, int n_pos, const float* custom_table,
                              int n_custom, const int* custom_map, int n_map, void* out, int* src_map, int C, hcpStream_t stream);
/* grad[k, :] (beta 1: +)= sum over the M rows m with src_map[m] == -1 - k of dX[m, :] (bf16 [M, C]), summed in increasing m by one
 * workgroup per (k, 256-column slab): no atomics, bit-reproducible.  grad fp32 [n_custom, C]. */
int hcp_embedding_pt_bwd_f32(const void* dX, const int* src_map, long M, int C, float* grad, int n_custom, int beta, hcpStream_t stream);
/* SDXL's second text encoder (CLIPTextModelWithProjection, "clip_bigG"; cfgs/train/examples/lora_sdxl.yaml trains LoRA on it).
 * hcp_gelu: its MLP activation (hidden_act "gelu": exact erf GELU), same calling shape as hcp_quick_gelu; any n > 0 (16-byte body,
 * scalar tail), 16-byte aligned buffers. */
int hcp_gelu(const void* x, const void* dy, void* out, long n, hcpStream_t stream);   /* dy NULL: forward; else dx */
/* Pooled output: pooled[b, :] = mean over the R chunks k of text_projection(final_layer_norm(x[b*R + k, eos, :])) (TEEXHook.forward_hook,
 * hcpdiff/models/textencoder_ex.py:73-76), eos = the FIRST position of the row's maximum id (transformers' rule for eos_token_id == 2).
 * x bf16 [B*R, L, C] (last layer's hidden states), ids int64 [B*R, L], gamma / beta fp32 [C], W = text_projection.weight [P, C]
 * (bf16, or fp32 with w_is_f32), pooled fp32 [B, P]; also written: positions int32 [B*R] and stats fp32 [B*R, 2] = (mean, rstd) of
 * the chosen token, which the backward reads.  One workgroup per (prompt, 16 output columns); no atomics.  C % 8 == 0, C <= 8192. */
int hcp_clip_pool_fwd(const void* x, const long long* ids, const float* gamma, const float* beta, const void* W, int w_is_f32,
                      float* pooled, int* positions, float* stats, int B, int R, int L, int C, int P, float eps, hcpStream_t stream);
/* dx bf16 [B*R, L, C] is WRITTEN (not added to): zero everywhere except row positions[m] of each m, which holds the LayerNorm
 * backward of W^T d_pooled[m / R] / R.  gamma and W are constants here (no gradient for final_layer_norm / text_projection).
 * One workgroup per row m, column sums in a fixed order: bit-reproducible.  C % 8 == 0, C + P <= 8192. */
int hcp_clip_pool_bwd(const void* x, const int* positions, const float* stats, const float* gamma, const void* W, int w_is_f32,
                      const float* d_pooled, void* dx, int B, int R, int L, int C, int P, hcpStream_t stream);
/* per-sample loss weights of the reference's timestep-aware criteria (hcpdiff/loss/min_snr_loss.py): kind 0 MinSNRLoss :21-25,
 * 1 SoftMinSNRLoss :31-35, 2 KDiffMinSNRLoss :39-43, 3 EDMLoss :47-52; snr = acp/(1-acp) as in :14-19.  w: float[B]. */
int hcp_snr_loss_weight(const long long* timesteps, const float* alphas_cumprod, float* w, int B, int kind, float gamma,
                        hcpStream_t stream);
/* (criterion(pred, target[, timesteps]) * mask).mean() * weight and its gradient (train_ac.py:506-515); criterion = MSE
 * (reduction none) times the optional per-sample weight sample_weight[B] (null: plain MSELoss) */
int hcp_mse_masked_mean(const float* pred, const float* target, const float* mask, int mask_channels,
                        const float* sample_weight, float* loss, float* grad, int B, int C, int HW, float weight,
                        hcpStream_t stream);
/* DreamArtist (reference models/cfg_context.py:12-39 + train_ac.py:506-515): the loss on the classifier-free-guidance combination of a
 * negative and a positive pass, and the gradient of both, in one streaming pass.  pred2 fp32 [2B, C, HW]: the negative ("uncond") rows
 * first, then the positive rows; target fp32 [B, C, HW]; mask (null, or 1 / C channels) and sample_weight (null or float[B]) as in
 * hcp_mse_masked_mean.  Per sample s_b = (cfg_hi - cfg_lo) rate_b + cfg_lo with r = timesteps[b] / (num_train_timesteps - 1) and
 * rate_b = r (rate_kind 0, 'ln'), cos((r - 1) pi / 2) (1, 'cos'), 1 - cos(r pi / 2) (2, 'cos2'); cfg_lo == cfg_hi is a fixed scale
 * (timesteps may be null).  e_b = u_b + s_b (c_b - u_b);  *loss = weight * mean((e - target)^2 * mask * sample_weight[b]) over B*C*HW;
 * grad2 (optional, [2B, C, HW]) = d loss / d pred2: with g = 2 weight / (B C HW) (e - target) mask sample_weight[b] the negative rows
 * get (1 - s_b) g, the positive rows s_b g.  partials: HCP_CFG_MSE_PARTIALS floats of workspace, one per workgroup, added in index
 * order by a second launch: no atomics, no memset, loss and gradient carry the same bits on every run.  The loss side (s_b, the
 * differences, squares and sums) is computed in double and rounded to fp32 twice, in the partial and in *loss; grad2 is fp32 arithmetic.
 * 16-byte loads and stores when HW % 4 == 0 and the buffers are 16-byte aligned, a scalar path otherwise. */
#define HCP_CFG_MSE_PARTIALS 2048
int hcp_cfg_mse_masked_mean(const float* pred2, const float* target, const float* mask, int mask_channels,
                            const float* sample_weight, const long long* timesteps, float cfg_lo, float cfg_hi, int rate_kind,
                            int num_train_timesteps, float* loss, float* grad2, float* partials, int B, int C, int HW, float weight,
                            hcpStream_t stream);

/* out[p,q] (+)= scale * sum_m L[m,p] R[m,q]  (fp32 atomics): the rank-r LoRA weight gradients
 * dW_down = alpha (dY W_up)^T x, dW_up = alpha dY^T (x W_down^T) (autograd of lora_base_patch.py:61-74). */
/* l_lo: 0, or the column offset of the residual half of a split L = (L_hi | L_lo) (hcp_gemm_lora_bf16 with ldt = 64: l_lo = 32): the
 * product is then (L_hi + L_lo)^T R. */
int hcp_lora_wgrad(const void* L, int ldl, int l_lo, const void* R, int ldr, float* out, int ldo, int M, int P, int Q, float scale,
                   int transpose_out, void* workspace, size_t workspace_bytes, hcpStream_t stream);
/* both gradients of one LoRA layer in one launch: grad_down[r,K] += s U^T x ; grad_up[N,r] += s dY^T T  (ldu / ldt: 32, or 64 = split) */
int hcp_lora_wgrad_pair(const void* U, int ldu, const void* x, int ldx, int K, float* grad_down, const void* T, int ldt, const void* dY,
                        int ldy, int N, float* grad_up, int M, int r, float scale, void* workspace, size_t workspace_bytes,
                        hcpStream_t stream);
/* dst[M,2C] bf16 = (bf16(src) | bf16(src - bf16(src))), src [M,C] fp32: the split form of a T / U produced by a GEMM of its own */
int hcp_split_hi_lo_bf16(const float* src, void* dst, long M, int C, hcpStream_t stream);
/* the weight gradients of MANY LoRA layers in two launches: partial tiles, ordered reduce (descriptor layout: csrc/lora.hip
 * WgradGroupDesc, 152 B; total_tiles = sum of qt_down + qt_up; slab_units = sum of blocks * P over the layers with more than one
 * token range: the workspace holds slab_units * 512 bytes; a layer with one range adds its tile itself).
 * No atomics anywhere on this path: every gradient element is summed in a fixed order by one thread (ABI 2; ABI 1 accumulated the
 * partials with fp32 atomics and took no workspace). */
int hcp_lora_wgrad_group_geometry(int M, int K, int N, int P, int target_blocks, int* qt_down, int* qt_up, int* splits,
                                  int* rows_per_split);
int hcp_lora_wgrad_group_desc_bytes(void);
int hcp_lora_wgrad_grouped(const void* descs, int count, int total_blocks, int total_tiles, long slab_units, void* workspace,
                           size_t workspace_bytes, hcpStream_t stream);
/* fp32 LoRA factors -> the four bf16 operand layouts, all layers in one launch (descs: device array, 80 B each, see
 * hcp_lora_pack_desc_bytes(): {const float* w_down; const float* w_up; bf16* ad; bf16* adt; bf16* bu; bf16* but; int K; int N; int r;
 * float alpha; int slot0; int n0; int Ntot; int bu_ld;} — slot0 / n0 / Ntot place a layer inside operand images shared by a fused
 * group; bu_ld = row stride of bu in elements (0 = 32); adt / but may be NULL when that image is not wanted) */
int hcp_lora_pack(const void* descs, int count, hcpStream_t stream);
int hcp_lora_pack_desc_bytes(void);

/* accelerator.clip_grad_norm_ + torch.optim.AdamW.step + zero_grad (train_ac.py:485-494) on one flat fp32 bucket. */
int hcp_sumsq_f32(const float* g, long n, float* out, hcpStream_t stream);
int hcp_adamw_clip_fused(float* p, float* g, float* m, float* v, long n, const float* lr, float beta1, float beta2,
                         float eps, float weight_decay, const float* sumsq, float grad_scale, float max_norm, int* step,
                         hcpStream_t stream);
/* hcp_sumsq_f32 without atomics: one partial per workgroup (partials: HCP_SUMSQ_PARTIALS floats), added in workgroup order by a second
 * launch.  The same bits on every run: with it a clip + Lion / Adafactor step is reproducible end to end. */
#define HCP_SUMSQ_PARTIALS 2048
int hcp_sumsq_ordered_f32(const float* g, long n, float* out, float* partials, hcpStream_t stream);
/* lion_pytorch.Lion (cfgs/train/examples/Lion_optimizer.yaml) on one flat fp32 bucket, conventions of hcp_adamw_clip_fused (grad_scale,
 * global-norm clip from *sumsq, device-resident lr, *step incremented, g left zero):
 * p *= 1 - lr wd;  p -= lr sign(beta1 m + (1 - beta1) g), sign(0) = 0;  m = beta2 m + (1 - beta2) g.  The betas are doubles: 1 - beta
 * is formed in double and rounded once. */
int hcp_lion_clip_fused(float* p, float* g, float* m, long n, const float* lr, double beta1, double beta2, float weight_decay,
                        const float* sumsq, float grad_scale, float max_norm, int* step, hcpStream_t stream);
/* transformers.optimization.Adafactor.step (cfgs/train/examples/FT_sdxl.yaml) for every tensor of one flat fp32 bucket, after the same
 * grad_scale / global-norm clip prologue; g is left zero, *step incremented.  descs = device array of `count` 112-byte rows
 * {long off, row_off, col_off, full_off, rowp_off, colp_off, s_outer, s_inner, s_r, s_c; int kind, outer, inner, R, C, item0, fitem0, pad;}
 * sorted by item0 (csrc/optim_factored.hip AfDesc; built by kernels.adafactor_table).  kind 0 VEC (1-D, unfactored: state in `full`),
 * 1 MAT (row-major [R, C]: `row` [R], `col` [C]), 2 TILE ([O, I, kh, kw], kh, kw <= 3, any dense strides: `row` [O, I, kh], `col`
 * [O, I, kw]).  m: first moments laid out as the bucket (NULL: beta1 None, the beta1 argument is then ignored).  workspace: the floats
 * the table asks for (one per work item, then the MAT tile partials); tstat: 4 floats per tensor, [0] = RMS(p) of the step; scal: 4
 * floats.  lr: device scalar (NULL with relative_step).  Seven launches whatever `count` is; no atomics: bit-reproducible. */
int hcp_adafactor_desc_bytes(void);
int hcp_adafactor_step(float* p, float* g, float* m, float* row, float* col, float* full, const void* descs, int count,
                       int total_items, int total_fitems, float* workspace, size_t workspace_bytes, float* tstat, float* scal,
                       const float* lr, float eps1, float eps2, float clip_threshold, float decay_rate, double beta1,
                       float weight_decay, int scale_parameter, int relative_step, int warmup_init, const float* sumsq,
                       float grad_scale, float max_norm, int* step, hcpStream_t stream);
/* ModelEMA.update (reference hcpdiff/utils/ema.py:17-27) over a flat bucket: ema <- lerp(ema, p, 1 - decay(step)) */
int hcp_ema_update(float* ema, const float* p, long n, const int* step, float inv_gamma, float power, float decay_max,
                   hcpStream_t stream);
/* bf16 wire formats of the sharded gradient / parameter exchange (what torch DDP's bf16_compress_hook does around its all-reduce,
 * torch/distributed/algorithms/ddp_comm_hooks/default_hooks.py; the reference reaches DDP through accelerate, train_ac.py:117-123):
 * dst_bf16[i] = bf16(src[i] * scale), src cleared when zero_src != 0 (the bucket's zero_grad);  dst_f32[i] = float(src_bf16[i]). */
int hcp_cast_f32_bf16(float* src, void* dst_bf16, long n, float scale, int zero_src, hcpStream_t stream);
int hcp_cast_bf16_f32(const void* src_bf16, float* dst, long n, hcpStream_t stream);

/* One DDIM (eta = 0) sampler step with classifier-free guidance fused in (reference utils/pipe_hook.py:120-140 + scheduler.step):
 * eps = eps2[:n] + g (eps2[n:] - eps2[:n]) when guided (eps2 = UNet output on [uncond ; cond]), else eps2[:n];
 * out = sqrt(a_prev) (x - sqrt(1 - a_t) eps) / sqrt(a_t) + sqrt(1 - a_prev) eps.  fp32, out may alias x. */
int hcp_cfg_ddim_step(const float* x, const float* eps2, float* out, long n, int guided, float guidance_scale,
                      float alpha_cumprod_t, float alpha_cumprod_prev, hcpStream_t stream);

/* Euler / Euler-ancestral sampling (diffusers EulerAncestralDiscreteScheduler / EulerDiscreteScheduler, epsilon prediction) with
 * classifier-free guidance, the legacy inpaint blend (utils/pipe_hook.py:429,442,453) and the next UNet input fused in (csrc/sampler.hip).
 * table: device float[steps][8], row i = (sigma_i, sigma_down_i, sigma_up_i, c_in_next_i, timestep_i, timestep_next_i, sigma_init_i,
 * c_in_i) with c_in = 1 / sqrt(sigma^2 + 1) and sigma_init the scale of a text2img start at row i; the final row of a run has
 * sigma_down = sigma_up = 0, c_in_next = 1 (sigma_down == 0 marks it).  state: device int64[2] = (seed, step); the kernels read row
 * state[1], clamped into the table, so no per-step value is an argument and one captured graph serves every step.
 * step:    eps = eps2[:n] + guidance (eps2[n:] - eps2[:n]) when guided, else eps2[:n];  x' = x + eps (sigma_down - sigma) + z sigma_up with
 *          z = noise[i], or (noise NULL) Box-Muller of Philox4x32-10 on counter (lo32, hi32 of i / 4, lo32(step), 0x53414D50), key (lo32,
 *          hi32 of seed), u = (w + 0.5) 2^-32, (z0, z1) = sqrt(-2 ln u0) (cos, sin)(2 pi u1), (z2, z3) from (u2, u3); nothing drawn when
 *          sigma_up == 0.  mask [B_rows,1,h,w] (hw = h w, chw = channels hw; needs init and noise0): x' = m (init + sigma noise0) +
 *          (1 - m) x', on the final row m init + (1 - m) x'.  x_out = x' (may alias x); model_in_next (nullable) [i] and, guided,
 *          [n + i] = c_in_next x'.  n % 4 == 0, 16-byte aligned fp32 buffers.
 * advance: state[1] <- min(state[1] + 1, steps - 1), t_out[0..rows) <- timestep of the new row (its own launch, after the step).
 * begin:   state[1] <- start_step, t_out <- its timestep, x <- z sigma_init (init NULL) or init + z sigma, z = noise[i] (may be x) or the
 *          draw with step word 0xFFFFFFFF; model_in (nullable) [i] and, guided, [n + i] = c_in x. */
int hcp_euler_step(const float* x, const float* eps2, float* x_out, float* model_in_next, long n, int B_rows, int guided, float guidance,
                   const float* table, int steps, const long long* state, const float* noise, const float* init, const float* noise0,
                   const float* mask, long chw, long hw, hcpStream_t stream);
int hcp_sampler_advance(long long* state, const float* table, int steps, long long* t_out, int rows, hcpStream_t stream);
int hcp_sampler_begin(long long* state, const float* table, int steps, float* x, float* model_in, long n, int guided, const float* noise,
                      const float* init, long long* t_out, int rows, int start_step, hcpStream_t stream);

/* (the tuning / ablation hooks of the -DHCP_TOOLS build are declared in include/hcp_mi355x_tools.h: they are not part of this ABI) */

/* ---- data-parallel exchange: RCCL over xGMI on flat buffers (csrc/comm.hip).  Replaces accelerator.backward's DDP gradient
 * all-reduce (reference train_ac.py:117-123,175,482).  One process per GPU; `comm` is an opaque handle owned by the caller;
 * every collective is stream-ordered, allocates nothing, never synchronises and can be captured into a hipGraph.
 * dtype: 0 = fp32, 1 = bf16.  RCCL is dlopen'ed on first use (the copy PyTorch-ROCm already mapped, if any). */
#define HCP_COMM_UNIQUE_ID_BYTES 128
int hcp_comm_unique_id(void* out128);                                   /* rank 0: create the 128-byte rendezvous token */
int hcp_comm_init(int rank, int world, const void* unique_id128, void** comm_out);   /* collective over all ranks */
int hcp_comm_destroy(void* comm);
int hcp_comm_rank(const void* comm);
int hcp_comm_world(const void* comm);
/* buf[i] <- sum over ranks, in place (one call per flat gradient bucket; 1/world is applied by hcp_adamw_clip_fused) */
int hcp_allreduce_flat(void* comm, void* buf, size_t count, int dtype, hcpStream_t stream);
/* recv[0..n) <- sum over ranks of send[rank*n .. rank*n+n)   (send: world*n elements) */
int hcp_reduce_scatter_flat(void* comm, const void* send, void* recv, size_t recv_count, int dtype, hcpStream_t stream);
/* recv[r*n .. r*n+n) <- rank r's send[0..n)   (recv: world*n elements; send may be its own slot of recv) */
int hcp_allgather_flat(void* comm, const void* send, void* recv, size_t send_count, int dtype, hcpStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
