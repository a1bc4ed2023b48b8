// hipzap native C ABI (consumed from Python through ctypes: hipzap/_native.py).
// Every struct here is mirrored field-for-field by a ctypes.Structure; keep them in sync.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { HZ_ACT_NONE = 0, HZ_ACT_RELU = 1, HZ_ACT_GELU = 2, HZ_ACT_TANH = 3 };

typedef struct HzConvParams {
  const unsigned short* x;   // input: channel-blocked [N][C/32][H][W][32] (C%32==0) or NHWC (C in {8,16})
  const unsigned short* w;   // fragment-major bf16 weights [Cout_pad/16][ksteps][64][8]; k = (r*S + s)*C + c
  const float* bias;         // fp32 [Cout] or NULL
  const unsigned short* res; // bf16 residual, same layout as out, or NULL
  void* out;                 // bf16 or fp32; channel-blocked, or row-major [M][ldo] if out_rowmajor
  int N, H, W, C;
  int Cout, R, S, stride, pad, P, Q;
  int M, K, ksteps;          // M = N*P*Q; ksteps = ceil(K/32)
  int act, out_f32, out_rowmajor, ldo;
  int x_rowmajor, ldx;        // GEMM mode: activations row-major [M][ldx] (M = N*H*W, 1x1 only)
  int tiles_n;               // filled by the launcher
  int kw;                    // waves per workgroup splitting K
  const struct HzLnFold* lnf; // LDS GEMM only: LayerNorm folded into this GEMM (device memory), or NULL
  // ResNet 1x1 -> 1x1 seams (block.hip seam_kernel; register-ring 3x3 convs only):
  int x_f32;                 // 1: x is fp32 in the same channel-blocked layout (a seam's conv1 sum, its
                             //    folded-BN bias included): ReLU + bf16 applied at the operand load
  int z_C;                   // channels of zinit
  float* zinit;              // or NULL: after its tiles the launch fills zinit [N][z_C/32][z_HW][32] fp32
                             //   with zbias[c] (the NEXT seam's accumulator, before its atomic adds)
  const float* zbias;        // [z_C]
  int z_HW, pad_z;
} HzConvParams;

// Post-LN transformer LayerNorm folded into the neighbouring GEMMs (gemm.hip, BERT). A GEMM
// whose input is LN(y) runs on the raw y with gamma folded into its weights (W' = W diag(gamma),
// c1[n] = sum_k W'[n][k], bias' = bias + W beta) and corrects in the epilogue:
//   out = rstd * (y.W'^T - mean * c1) + bias'
// A GEMM whose residual is LN(y) normalises the residual elementwise. The producing GEMM writes
// per-row partial (sum, sumsq) of its bf16-rounded output, one float2 slab per (N tile, wave
// column): deterministic, no atomics; consumers sum the slabs of a row.
typedef struct HzLnFold {
  const float* stats_in;   // [nslab_in][ld_stats] float2 of the GEMM input rows, or NULL
  const float* c1;         // [Cout] (with stats_in)
  const float* res_stats;  // [nslab_res][ld_stats] float2 of the residual rows, or NULL
  const float* res_gamma;  // [Cout] (with res_stats)
  const float* res_beta;
  float* stats_out;        // [2 * tiles_n][ld_stats] float2 of this GEMM's output rows, or NULL
  int nslab_in, nslab_res, ld_stats;
  float inv_d, eps_in, eps_res;  // inv_d = 1 / LayerNorm width
} HzLnFold;

// cfg 0..8: register-ring tile (FC*16 channels x FP*16 pixels), cfg = log2(FC)*3 + log2(FP);
// cfg 16..19: LDS-tiled GEMM (gemm.hip; row-major activations, K % 64 == 0, weight rows % 128 == 0)
int hz_conv_launch(const HzConvParams* p, int cfg, hipStream_t st);
int hz_gemm_lds_launch(const HzConvParams* p, int cfg, hipStream_t st);
// two independent convs with one shared (cfg, kw) in one launch (grouped; conv.hip conv2_kernel)
int hz_conv2_launch(const HzConvParams* a, const HzConvParams* b, int cfg, hipStream_t st);

typedef struct HzPoolParams {
  const unsigned short* x;  // NHWC bf16
  unsigned short* out;      // NHWC bf16
  int N, H, W, C, P, Q, k, stride, pad;
} HzPoolParams;
int hz_maxpool_launch(const HzPoolParams* p, hipStream_t st);
// global average pool NHWC [N,H,W,C] -> [N,C] bf16
// blocked: x is [N][C/32][HW][32] instead of NHWC
int hz_avgpool_launch(const unsigned short* x, unsigned short* out, int N, int HW, int C, int blocked, hipStream_t st);

// fused global-average-pool + classifier (ResNet head):
//   out[b][n] = bias[n] + sum_c W[n][c] * mean_hw x[b][c][hw]
typedef struct HzPoolFcParams {
  const unsigned short* x;  // channel-blocked bf16 [B][C/32][HW][32]
  const unsigned short* w;  // fragment-major bf16 [N_pad/16][C/32][64][8] (pack_linear)
  const float* bias;        // [N]
  float* out;               // fp32 [B][ldo]
  int B, C, HW, N, ldo;
  int pooled, pad_;         // pooled: x is already the fp32 [B][C] channel means (a tail seam's output)
} HzPoolFcParams;
int hz_pool_fc_launch(const HzPoolFcParams* p, hipStream_t st);

// global average pool [+ L2 normalisation] without the classifier (ResNet embedding head, DESIGN.md 4r;
// vision.hip pool_norm_kernel): out[b][c] = mean_hw x[b][c][hw] in fp32, the sum in ascending pixel order
// times 1.f / HW (pool_fc_kernel's channel mean, bit for bit); normalize: divided by max(||row||_2, 1e-12).
// One workgroup per image, no atomics: a row's bits depend on that image alone. Columns C..ldo-1 of out
// are left as they were. Refused (-1, nothing launched): x or out null or not 16-B aligned, B < 1, HW < 1,
// C < 32, C % 32, C > 2048, ldo < C.
typedef struct HzPoolNormParams {
  const unsigned short* x;  // channel-blocked bf16 [B][C/32][HW][32]; pooled: fp32 [B][C] channel means
  float* out;               // fp32 [B][ldo]
  int B, C, HW, ldo;
  int pooled, normalize;    // pooled: as HzPoolFcParams.pooled (then, without normalize, a bitwise copy)
} HzPoolNormParams;
int hz_pool_norm_launch(const HzPoolNormParams* p, hipStream_t st);

// image pre-processing: src NCHW fp32 (mode 0) or NHWC uint8 (mode 1) -> NHWC bf16 with Cpad channels;
// mode 2: src NCHW fp32 -> bf16 patch rows [N * H/P * W/P][Cin * P * P] in (c, ky, kx) order, with
// P = Cpad (16; the ViT patch embedding as a row-major GEMM)
int hz_preprocess_launch(const void* src, unsigned short* dst, int N, int Cin, int H, int W, int Cpad,
                         int mode, const float* mean, const float* inv_std, hipStream_t st);

// resize + centre crop + normalise in one launch (vision.hip resize_preprocess_kernel): a uint8 HWC image
// of any size up to maxH x maxW -> bf16 NHWC8 [B][crop][crop][8]. The resize is torch's antialiased
// bilinear (triangle filter of support max(in/out, 1), weights normalised by their sum, fp32). The grid
// depends on B and crop only: the per-request geometry is read from `dims` at run time, so one captured
// graph serves every image size. Every index is clamped: no header makes a read leave its row of `image`.
typedef struct HzResizeParams {
  const unsigned char* image;  // [B][cap_bytes] uint8, a tightly packed H x W x 3 image at each row's start
  const int* dims;             // [B][8] {H, W, rh, rw, top, left, 0, 0}: source size, resized size, crop origin
  unsigned short* out;         // [B][crop][crop][8] bf16, channels 3..7 zero
  int B, crop, maxH, maxW;
  long long cap_bytes;         // bytes per row of `image`: >= maxH * maxW * 3, a multiple of 16
  float mean[4], inv_std[4];   // (x / 255 - mean) * inv_std
} HzResizeParams;
int hz_resize_preprocess_launch(const HzResizeParams* p, hipStream_t st);
// The same resize, crop and normalisation written as ViT patch rows (vision.hip resize_patchify_kernel):
// `out` is bf16 [B * n * n][3 * 16 * 16], n = crop / 16; pixel (oy, ox) channel c of image b is column
// c * 256 + (oy % 16) * 16 + ox % 16 of row (b * n + oy / 16) * n + ox / 16 (the patchify layout, the
// patch-embed GEMM's operand). The same value per pixel as the NHWC8 kernel, bit for bit. Also refuses
// a crop that is no multiple of 16 or below 16.
int hz_resize_patchify_launch(const HzResizeParams* p, hipStream_t st);

// elementwise helpers
int hz_cast_f32_bf16(const float* x, unsigned short* y, long n, hipStream_t st);
int hz_cast_bf16_f32(const unsigned short* x, float* y, long n, hipStream_t st);

typedef void* HzProgram;

// ---- AWD-LSTM decode (csrc/lstm.hip) ----
typedef struct HzLstmParams {
  const unsigned short* w;    // [4H][ldk] bf16, gate-interleaved rows (4j+q = gate q of unit j; i,f,g,o)
  const float* bias;          // [4H] fp32 (b_ih + b_hh, same interleave)
  const unsigned short* emb;  // layer 0: embedding [V][lde] bf16 (input gathered by token); else NULL
  int lde;
  int* tok_seq;               // token sequence; step t consumes tok_seq[t]
  const float* x_state;       // layers > 0: previous layer's h_state [2][In]
  float* h_state;             // [2][H] fp32, ping-pong by step parity
  float* c_state;             // [2][H] fp32
  const int* step;            // device step counter: this op runs step t = *step + step_off
  int In, H, ldk;             // ldk = padded In + H (multiple of 64; chunks of 512 are predicated)
  int step_off;
  // layer 0 only, optional (fused sampler): for t >= *n_forced the token of step t is the argmax
  // of the previous step's decoder maxima (the argmax sampler's rule, computed redundantly by
  // every workgroup); workgroup 0 records it in tok_seq[t]. NULL bacc_val: tok_seq[t] is read.
  const int* n_forced;
  const float* bacc_val;      // [nblk] decoder per-workgroup maxima over acceptable rows
  const int* bacc_idx;
  const float* bmax_val;      // [nblk] overall maxima (fallback when no row is acceptable)
  const int* bmax_idx;
  int nblk, V;
  // split mode (pre != NULL; csrc/lstm.hip lstm_x_kernel): w holds W_ih only ([4H][ldk], ldk =
  // In padded to 64) and the recurrent half arrives precomputed by the previous step's decoder
  // kernel: pre[4H] = W_hh . h_{t-1} + b (bias is then unused)
  const float* pre;
  // split mode, layer 0 folded into the layer-1 kernel (xtab != NULL; In = H0): h0_t is rebuilt
  // in every workgroup from xtab[tok] (= W_ih^0 . emb[tok], fp32 [V][4*H0]), pre0 and c0_{t-1};
  // token selection as above (emb unused); workgroup 0 publishes h0_t / c0_t
  const float* xtab;
  const float* pre0;          // [4*H0]
  float* h0_state;            // [2][H0]
  float* c0_state;            // [2][H0]
  int H0, pad0;
} HzLstmParams;
typedef struct HzSamplerParams {
  const float* keys;          // [V] Gumbel-perturbed logits (decoder epilogue)
  int* tok_seq;               // writes tok_seq[t+1] when t+1 >= n_forced
  const int* step;            // this op samples after step t = *step + step_off (no increment:
  int step_off;               //   hz_step_bump_launch advances the counter once per graph)
  int* draws;                 // optional [steps][10] record of the draws
  const int* n_forced;        // device: prompt length (tokens 0..n_forced-1 are given)
  int V, n_exclude;
  int exclude[8];
  const float* bmax_val;      // [nblk] decoder workgroup maxima (value, row)
  const int* bmax_idx;
  int nblk, rpb;              // decoder geometry: workgroup b owns rows [b*rpb, (b+1)*rpb)
  // with draws == NULL: the token is the argmax of the ACCEPTABLE keys (row != 0, not excluded),
  // from the decoder's per-workgroup acceptable maxima; exact for the reference rule (see lstm.hip)
  const float* bacc_val;      // [nblk] or NULL (then the top-10 tournament always runs)
  const int* bacc_idx;
} HzSamplerParams;
typedef struct HzDecoderParams {
  const unsigned short* w;    // [V][ldk] bf16 (tied embedding, K padded)
  const float* bias;          // [V] or NULL
  const float* h_state;       // last layer [2][H]
  const int* step;            // step t = *step + step_off
  int step_off;
  float* logits;              // [V]
  int V, H, ldk;
  float* keys;                // optional [V]: logits + Gumbel(seed, step, row) for the sampler
  const unsigned long long* seed;
  float* bmax_val;            // with keys: [nblk] per-workgroup max key (value, row) -> sampler
  int* bmax_idx;
  int nblk, rpb;              // workgroups and rows per workgroup (hz_decoder_geometry)
  float* bacc_val;            // optional [nblk]: per-workgroup max key over ACCEPTABLE rows
  int* bacc_idx;              //   (row != 0 and not in exclude[]), -inf/INT_MAX if none
  int n_exclude;
  int exclude[8];
  // split LSTM mode: hh_blocks extra workgroups (blockIdx < hh_blocks, before the decoder's)
  // compute the NEXT step's recurrent gate partials hh_out[l] = W_hh^l . h^l_t + b^l, layer l
  // owning workgroups [hh_blk[l], hh_blk[l+1]) of HZ_HH_ROWS rows each
  int n_hh, hh_blocks;
  const unsigned short* hh_w[4];  // [4H][ld] bf16, gate-interleaved like HzLstmParams.w
  const float* hh_b[4];           // [4H]
  const float* hh_h[4];           // the layer's h_state [2][H]
  float* hh_out[4];               // [4H] -> HzLstmParams.pre / pre0
  int hh_H[4], hh_ld[4];
  int hh_blk[5];
} HzDecoderParams;
#define HZ_HH_ROWS 16
// decoder launch geometry for vocabulary V: workgroups and rows per workgroup (contiguous)
void hz_decoder_geometry(int V, int* nblk, int* rpb);
int hz_lstm_cell_launch(const HzLstmParams* p, hipStream_t st);
int hz_decoder_launch(const HzDecoderParams* p, hipStream_t st);
int hz_sampler_launch(const HzSamplerParams* p, hipStream_t st);
// *step += n (one thread): closes a captured run of decode steps
int hz_step_bump_launch(int* step, int n, hipStream_t st);

// ---- batched AWD-LSTM decode (csrc/lmbatch.hip + csrc/lmserve.cpp) ----
// Continuous batching for concurrent GET /inference: Bp (16 or 32) request rows share every
// decode step, so each weight byte is read once per step for all of them. Weights and the
// recurrent state are fragment-major for mfma_f32_16x16x32_bf16: W as the A operand
// ([R/16][K/32][64 lanes][8], lane l = row l&15, k 8(l>>4)..+7) and h as the B operand
// ([K/32][Bp/16][64][8], lane l = request row l&15). h is kept as a bf16 hi/lo pair (hi = bf16(h),
// lo = bf16(h - hi)): two MFMAs per fragment give ~16 mantissa bits of the fp32 state.
// Per-step control comes from the host scheduler (row step, forced prompt token or sample, where
// the token goes): the admit kernel copies it from a pinned host block at each replay start.
#define HZ_LMB_MAXU 32
typedef struct HzLmbCtl {     // one (sub-step u, row r) entry, computed by the host
  int tok;                    // >= 0: forced (prompt) token; -1: sample from the last decoder; -2: idle row
  int out;                    // sampled token's index in the request's output (-1: none)
  int dec_t;                  // decoder: step t whose next token is sampled (noise counter), -1: no keys
  int rec;                    // decoder: 1 = record this row's logits (tests)
} HzLmbCtl;
typedef struct HzLmbLayerParams {
  const unsigned short* w;    // [R/16][(Kh+Kx)/32][64][8] bf16, K order [h_prev | x], rows 4j+q (gate q of unit j)
  const float* bias;          // [R] fp32 (b_ih + b_hh, same interleave)
  unsigned short* h;          // this layer's state [2 parity][2 hi/lo][Kh/32][Bp/16][64][8] bf16
  const unsigned short* x;    // layers > 0: the previous layer's h buffers (its Kh = this Kx)
  float* c;                   // [Bp][H] fp32 cell state
  const int* gpar;            // device: h parity of the graph's first sub-step
  const HzLmbCtl* ctl;        // [U][Bp] (first layer)
  int H, Kh, Kx, R, Bp, step_off;
  // first layer: the token of each row (forced, or the argmax of the previous decoder's maxima)
  // and its embedding as the x operand
  const unsigned short* emb;  // [Vp/16][Kx/32][64][8] fragment-major embedding (NULL: not first)
  unsigned long long* dbest;  // [2 parity][Bp] running maxima (packed key, row) of the decoder; the
  int V;                      //   first layer reads the other parity and clears its own
  int nb_act;                 // row blocks (of 16) computed: 0 = all Bp/16; 1 = rows 0..15 only (the
                              //   low-load program: every busy row is below 16); -1 = request row 0
                              //   only (the one-request program: no other row's state read or written)
  int* const* outp;           // [Bp] request output arrays (pinned host, written by workgroup 0)
  int* tok;                   // [Bp] this step's tokens (device, diagnostics)
  const float* embproj;       // first layer: [Vp][R] fp32 W_ih E[v] (hz_lmb_embproj_launch) or NULL
} HzLmbLayerParams;
typedef struct HzLmbEmbProjParams {  // P[v][r] = sum_k W[r][Kh + k] emb[v][k]
  const unsigned short* w;    // the first layer's packed weights [R/16][(Kh+Kx)/32][64][8]
  const unsigned short* emb;  // [Vp/16][Kx/32][64][8]
  float* out;                 // [Vp][R]
  int R, Kh, Kx, Vp;
} HzLmbEmbProjParams;
typedef struct HzLmbDecParams {
  const unsigned short* w;    // [Vp/16][K/32][64][8] bf16 (tied embedding when untied weights are absent)
  const float* bias;          // [Vp] or NULL
  const unsigned short* h;    // last layer's h buffers (Kh = K)
  const int* gpar;
  const HzLmbCtl* ctl;        // [U][Bp]
  const unsigned long long* seed;  // [Bp]
  unsigned long long* dbest;  // [2 parity][Bp]: atomic max over acceptable ids -> the next first layer
  float* logits;              // [Bp][V] (recorded rows only) or NULL
  int V, Vp, K, Bp, nblk, step_off, n_exclude;
  int nb_act;                 // as HzLmbLayerParams::nb_act
  int exclude[8];
} HzLmbDecParams;
typedef struct HzLmbAdmitParams {
  const int* block;           // pinned host block (csrc/lmserve.cpp layout)
  HzLmbCtl* ctl;              // [U][Bp] device
  unsigned long long* seed;   // [Bp]
  int** outp;                 // [Bp]
  int* gpar;
  int Bp, U, n_layers, pad_;
  unsigned short* h[4];       // per layer: h buffers (zeroed for an admitted row)
  float* c[4];                // [Bp][H]
  int Kh[4], H[4];
} HzLmbAdmitParams;
int hz_lmb_layer_launch(const HzLmbLayerParams* p, hipStream_t st);
int hz_lmb_dec_launch(const HzLmbDecParams* p, hipStream_t st);
int hz_lmb_admit_launch(const HzLmbAdmitParams* p, hipStream_t st);
int hz_lmb_embproj_launch(const HzLmbEmbProjParams* p, hipStream_t st);
int hz_lmb_dec_blocks(int V);  // decoder workgroups (256 vocabulary rows each)
// scheduler: one worker thread replays the captured U-step program(s); requests join free rows
// at replay boundaries and leave when their last token is out (csrc/lmserve.cpp). Two programs
// (each reading its own host block and recording into its own logits buffer): pipelined replays.
void* hz_lmb_create(const HzProgram* progs, int nprog, hipStream_t st, int* const* blocks, int Bp, int U, int maxp,
                    int maxn, int* out_pool, float* const* logits, int V);
int hz_lmb_submit(void* s, const int* prompt, int P, int n, unsigned long long seed, int* out, float* logits_out,
                  double* lat_us);
void hz_lmb_stats(void* s, unsigned long long* out4);  // replays, served, row-steps used, row-steps total
int hz_lmb_set_lowload(void* s, const HzProgram* lo, int rows);  // programs for replays whose busy rows are < rows
unsigned long long hz_lmb_lo_replays(void* s);
int hz_lmb_set_solo(void* s, const HzProgram* solo);  // programs for replays whose only busy row is row 0
unsigned long long hz_lmb_solo_replays(void* s);
void hz_lmb_destroy(void* s);

// ---- device-side packing of raw checkpoint tensors (csrc/pack.hip; torch-free .pth cold start) ----
typedef struct HzPackConvParams {
  const float* w;             // OIHW fp32, contiguous (a Linear weight is [cout][cin] with r = s = 1)
  const float* gamma;         // eval BatchNorm (fp32 [cout]) to fold, or NULL
  const float* beta;
  const float* mean;
  const float* var;
  const float* bias_in;       // [cout] or NULL
  unsigned short* wf;         // packed bf16 [rows/16][ksteps][64][8]
  float* bias_out;            // [cout] fp32
  int cout, cin, r, s, cin_p, rows, ksteps, pad_;
  double eps;
} HzPackConvParams;
int hz_pack_conv_launch(const HzPackConvParams* p, hipStream_t st);
int hz_conv_code_warm(void);    // load conv.hip / vision.hip device code (no launch)
int hz_vision_code_warm(void);
int hz_gemm_code_warm(void);
int hz_transformer_code_warm(void);
int hz_fp8_code_warm(void);
int hz_pack_code_warm(void);
// fp32 row-major source(s) -> bf16 fragment-major [R/16][K/32][64][8] (+ an fp32 bias row), the
// batched AWD-LSTM packing (engine/lmbatch.py pack_lmb) on the device: output row r reads source
// row r, or (interleave_h = H > 0) row (r & 3) * H + (r >> 2) (unit-major gates); output column k
// reads a[src][k] for k < ka (zero at k >= acols) and b[src][k - ka] beyond (zero at >= bcols);
// source rows >= nrows and absent segments are zeros. out == NULL: bias only.
typedef struct HzFragPackParams {
  const float* a;
  const float* b;
  unsigned short* out;
  const float* bias_a;  // bias_out[r] = bias_a[src] (+ bias_b[src]), zero beyond the source rows
  const float* bias_b;
  float* bias_out;
  int R, K, nrows, interleave_h, ka, acols, lda, bcols, ldb, pad_;
} HzFragPackParams;
int hz_frag_pack_launch(const HzFragPackParams* p, hipStream_t st);
// file byte ranges -> device memory (csrc/plan.cpp): pread into two pinned staging buffers, DMA
// chunk i while reading chunk i+1; synchronous on `st`
int hz_upload_file(const char* path, int n, const uint64_t* file_off, const uint64_t* nbytes, void* const* dst,
                   void* st);

// ---- FP8 (OCP e4m3fn) path (csrc/fp8.hip) ----
typedef struct HzQuantParams {
  const unsigned short* x;    // [rows][ldx] bf16
  unsigned char* out;         // [rows][ldo] fp8 e4m3fn
  float* scale;               // [rows] fp32 (amax/448)
  int rows, D, ldx, ldo;
} HzQuantParams;
typedef struct HzGemmFp8Params {
  const unsigned char* x;     // [M][ldx] fp8
  const float* sx;            // [M] row scales
  const unsigned char* w;     // fragment-major fp8 [N_pad/16][ksteps][64][8]
  const float* sw;            // [N_pad] per-channel scales
  const float* bias;          // [N] or NULL
  const unsigned short* res;  // [M][ldo] bf16 or NULL
  void* out;                  // [M][ldo] bf16 or fp32
  int M, N, K, ksteps, ldx, ldo;
  int act, out_f32, cfg, kw;
  const unsigned char* wmx;   // MX-packed weights [N_pad/16][K/128][2][64][16] (cfg 16..23) or NULL
  // MX8 activations (OCP MX: e4m3 + one E8M0 power-of-two scale per 32 consecutive k), cfg >= 16:
  const unsigned char* xs;    // input block scales [M][K/32] (then sx may be NULL) or NULL
  unsigned char* out8;        // MX8 output instead of `out`: e4m3 [M][ldo] ...
  unsigned char* os8;         //   ... and E8M0 scales [M][ldo/32]
} HzGemmFp8Params;
int hz_quant_launch(const HzQuantParams* p, hipStream_t st);
int hz_gemm_fp8_launch(const HzGemmFp8Params* p, hipStream_t st);

// ---- transformer kernels (csrc/transformer.hip) ----
typedef struct HzLayerNormParams {
  const unsigned short* x;    // [rows][ldx] bf16
  const unsigned short* res;  // optional residual [rows][ldr] (added before the norm)
  unsigned short* out;        // [rows][ldo] bf16
  const float* gamma;
  const float* beta;
  int rows, D, ldx, ldr, ldo;
  float eps;
  unsigned char* out8;        // optional fused per-row fp8 quantisation of the output [rows][D]
  float* scale8;              //   and its row scales (amax / 448); out may then be NULL
} HzLayerNormParams;
typedef struct HzEmbedParams {
  const int* ids;             // [rows] token ids (rows = B*L)
  const int* types;           // [rows] token-type ids or NULL
  const unsigned short* word; // [V][D]
  const unsigned short* pos;  // [Lmax][D]
  const unsigned short* type; // [2][D]
  const float* gamma;
  const float* beta;
  unsigned short* out;        // [rows][D]
  int rows, L, D;
  float eps;
  int vocab, ntypes;          // table rows: ids / types are clamped into range (a bad request id
                              // cannot read outside the tables; the servers also reject it)
} HzEmbedParams;
typedef struct HzAttentionParams {
  const unsigned short* qkv;  // [B*L][ldqkv]: Q at col h*64, K at +k_off, V at +v_off
  const float* mask;          // additive per-key mask [B][L] or NULL
  unsigned short* out;        // [B*L][ldo], head h at col h*64
  int B, L, heads, head_dim, ldqkv, k_off, v_off, ldo;
  float scale;
  unsigned char* out8;        // optional MX8 output (e4m3 [B*L][ldo] + E8M0 [B*L][ldo/32]) instead of out
  unsigned char* os8;
} HzAttentionParams;
typedef struct HzVitTokensParams {
  const unsigned short* patches;  // [B*np][D]
  const unsigned short* cls;      // [D]
  const unsigned short* pos;      // [np+1][D]
  unsigned short* out;            // [B][np+1][D]
  int B, np, D;
} HzVitTokensParams;
int hz_layernorm_launch(const HzLayerNormParams* p, hipStream_t st);
int hz_embed_ln_launch(const HzEmbedParams* p, hipStream_t st);
int hz_attention_launch(const HzAttentionParams* p, hipStream_t st);
// QKV projection + self-attention in one launch (transformer.hip qkvatt_kernel): one workgroup per
// (sequence, head), L <= 128, head_dim 64; the QKV GEMM's own weight packing and bias
typedef struct HzQkvAttParams {
  const unsigned short* x;    // [B*L][ldx] bf16 (the layer input)
  const unsigned short* w;    // packed QKV weights [3D/16][D/32][64][8] (rows: Q 0..D-1, K D.., V 2D..)
  const float* bias;          // [3D]
  const float* mask;          // additive per-key mask [B][L] or NULL
  unsigned short* out;        // [B*L][ldo] context, head h at column h*64
  int B, L, heads, D, ksteps, ldx, ldo;
  float scale;
} HzQkvAttParams;
int hz_qkvatt_launch(const HzQkvAttParams* p, hipStream_t st);
int hz_vit_tokens_launch(const HzVitTokensParams* p, hipStream_t st);
// pooled embeddings (transformer.hip pool_embed_kernel): the final hidden states -> one fp32 vector per
// sequence in one launch. mode 0: the CLS row (row b*L; mask and first ignored); mode 1: the mean of the
// counted tokens of [first, L), a token counting iff its additive mask value is 0 (the hosts write 0 or
// -1e9; NULL mask: all count). normalize: divide by max(||v||_2, 1e-12) in fp32. A sequence with no
// counted token gives a zero row. One workgroup per sequence, fp32 sums in a fixed order, no atomics: a
// sequence's output bits do not depend on B, on its row or on the other rows.
typedef struct HzPoolEmbedParams {
  const unsigned short* x;    // [B*L][ldx] bf16, D columns used (16-B aligned, ldx % 8 == 0)
  const float* mask;          // additive mask [B][L] or NULL
  float* out;                 // [B][ldo] fp32; columns D..ldo-1 are written as zero
  int B, L, D, ldx, ldo;      // D % 8 == 0, D <= 2048
  int first, mode, normalize;
} HzPoolEmbedParams;
int hz_pool_embed_launch(const HzPoolEmbedParams* p, hipStream_t st);

// ---- vector search (csrc/search.hip, csrc/index.cpp): exact top-k by inner product ----
// scan: one workgroup per tile of HZ_SEARCH_TILE corpus rows scores every row of its tile against all Q
// queries (fp32 FMAs over the fp32 query and the bf16 row widened to fp32) and writes the tile's best
// min(k, rows in tile) candidates per query, best first, as 64-bit keys; unused slots hold key 0.
// merge: one workgroup per query reduces its ntile x k keys to the final k, best first.
// Order (total): higher score first, then the lower row id. key = (orderable(score) << 32) | ~id with
// -0.0 canonicalised to +0.0; key 0 is below every real key and decodes to id -1, score -inf.
// The bits of score(q, r) depend on the D values of the query and of the row only.
#define HZ_SEARCH_TILE 256
#define HZ_SEARCH_MAX_Q 16
#define HZ_SEARCH_MAX_K 128
typedef struct HzSearchParams {
  const unsigned short* corpus;  // bf16 [N][ldc], 16-B aligned rows (ldc % 8 == 0), ldc >= D
  const float* queries;          // fp32 [Q][D], 16-B aligned
  unsigned long long* cand;      // scratch [ntile][Q][k] keys, at least hz_search_scratch_bytes(N, Q, k)
  float* out_score;              // fp32 [Q][k]
  int* out_id;                   // int32 [Q][k]
  int N, D, Q, k, ldc;
  int ntile;                     // filled by the launchers: ceil(N / HZ_SEARCH_TILE)
  unsigned long long cand_bytes; // bytes of `cand`
} HzSearchParams;
int hz_search_tile_rows(void);   // HZ_SEARCH_TILE
// bytes of candidate scratch a search of (N, Q, k) needs; 0 for a refused shape
unsigned long long hz_search_scratch_bytes(long long N, int Q, int k);
// 0, or a negative code for a refused parameter block (nothing is launched then)
int hz_search_scan_launch(const HzSearchParams* p, hipStream_t st);
int hz_search_merge_launch(const HzSearchParams* p, hipStream_t st);
// filtered scan (HZ_K_SEARCH_FSCAN): the scan over the rows that pass
//   pass(q, r) = live(r) && (filt == NULL || (tags[r] & filt[q][0]) == filt[q][1])
// A failing (q, r) scores the sentinel 0 (below every real key), whatever the row holds; a row that fails for
// every query of the launch is not loaded. A tile's list holds its passing rows' best k keys, then key 0.
// The score bits of a passing (q, r) are those of HZ_K_SEARCH_SCAN; HZ_K_SEARCH_MERGE reduces the lists.
typedef struct HzSearchFilterParams {
  HzSearchParams s;              // the scan's block, unchanged
  const unsigned* live;          // 1 bit per row: bit r & 31 of word r >> 5
  const unsigned* tags;          // one u32 per row [N], or NULL (then filt must be NULL)
  const unsigned* filt;          // device [Q][2] = {mask, value} per query, or NULL: no tag predicate
  unsigned long long live_bytes; // bytes of `live`, at least 4 * ceil(N / 32)
} HzSearchFilterParams;
int hz_search_fscan_launch(const HzSearchFilterParams* p, hipStream_t st);
// quantised scan (HZ_K_SEARCH_QSCAN): the filtered scan over rows of OCP e4m3fn bytes, one fp32 scale per row.
// `f.s.corpus` points at uint8 [N][ldc] (ldc in bytes, ldc % 16 == 0, D % 16 == 0, 16 <= D <= 2048).
//   score(q, r) = fl32(scales[r] * sum_i q_i * decode(code_ri)), the sum as in HZ_K_SEARCH_SCAN
// Its bits depend on the query's D values, the row's D codes and the row's scale only. The codes and the scale
// of a row that fails for every query are never loaded. HZ_K_SEARCH_MERGE reduces the lists.
typedef struct HzSearchQuantParams {
  HzSearchFilterParams f;        // the filtered scan's block, unchanged (live is required)
  const float* scales;           // fp32 [N], 4-B aligned
} HzSearchQuantParams;
int hz_search_qscan_launch(const HzSearchQuantParams* p, hipStream_t st);
// binary scan (HZ_K_SEARCH_BSCAN): the filtered scan over sign-bit rows. `f.s.corpus` points at
// uint32 [N][ldc] (ldc in WORDS, ldc % 4 == 0, ldc >= W = D / 32; D % 128 == 0, 128 <= D <= 2048): bit i & 31 of
// word i >> 5 of a row is 1 iff the sign bit of column i is clear (the live bitmap's bit convention; -0.0 gives 0).
// The kernel binarises the fp32 queries by the same rule and scores
//   score(q, r) = (float)(D - 2 * popcount(qbits ^ rbits)),
// an integer in [-D, D], exact in fp32; keys and the total order are HZ_K_SEARCH_SCAN's, so equal scores (the
// normal case: only D + 1 values exist) rank by the lower id. The bits of a score depend on the query's D sign bits
// and the row's W words, and on nothing else: not on N, Q, k, ldc, the row's tile or position, the other queries,
// the filter, or what dead rows hold. The words of a row that fails for every query are never loaded.
// HZ_K_SEARCH_MERGE reduces the lists. Filtered only: `live` is required.
// Refusals (nothing is launched): -80 a null corpus, queries, cand, out_score or out_id; -81 D % 128; -82 D < 128;
// -83 D > 2048; -84 ldc < D / 32 or ldc % 4; -85 N < 1 (N >= 2^31 cannot be expressed: hz_search_scratch_bytes
// refuses it); -86 Q outside 1..HZ_SEARCH_MAX_Q; -87 k outside 1..HZ_SEARCH_MAX_K; -88 corpus or queries not 16-B,
// cand not 8-B or out_* / tags / filt / live not 4-B aligned; -89 a null live bitmap; -90 live_bytes below
// 4 * ceil(N / 32); -91 filt without tags; -92 cand_bytes below ntile * Q * k * 8.
typedef struct HzSearchBinParams {
  HzSearchFilterParams f;        // the filtered scan's block, unchanged (live is required; ldc counts words)
} HzSearchBinParams;
int hz_search_bscan_launch(const HzSearchBinParams* p, hipStream_t st);
// product-quantised rows: the D columns are M sub-spaces of dsub = D / M columns; a row is M bytes,
// code[r][m] naming one of 256 sub-centroids codebook[m][c][0 .. dsub) (fp32 [M][256][dsub]). Shape rules, for both
// kinds: M % 16 == 0 (a row is whole 16-B chunks), 16 <= M <= HZ_SEARCH_PQ_MAX_M (one query's table is M KiB of
// LDS), D % M == 0, 1 <= D / M <= HZ_SEARCH_PQ_MAX_DSUB, D <= 2048.
// CONTRACT. lut[q][m][c] is ONE fp32 fmaf chain over j = 0 .. dsub-1, ascending, from +0, of
// q[m*dsub + j] * codebook[m][c][j]; score(q, r) is the fp32 sum, PLAIN additions (no FMA), over m = 0 .. M-1,
// ascending, from +0, of lut[q][m][code[r][m]]. The bits of a score depend on the query, the codebook and the row's
// M bytes only: not on N, the tile, the row's position, the other queries, the grid or `span`. Keys and the total
// order are HZ_K_SEARCH_SCAN's. Against the exact inner product of q and the reconstructed row x^:
//   |score - q.x^| <= gamma(dsub + M) * sum_i |q_i| |x^_i|,  gamma(n) = n 2^-24 / (1 - n 2^-24).
// table kind (HZ_K_SEARCH_PQLUT): grid (M, Q), 256 threads; thread c writes lut[(q*M + m)*256 + c].
// scan kind (HZ_K_SEARCH_PQSCAN): `f.s.corpus` points at uint8 [N][ldc] (ldc in bytes, ldc % 16 == 0, ldc >= M).
// Grid (ceil(ntile / span), Q): a workgroup copies ITS query's M KiB table from `lut` into LDS once and walks `span`
// consecutive tiles; per tile thread t owns row t, loads its M bytes only if the row passes for this query (a wave
// whose 64 rows all fail loads nothing), adds the M lookups and the tile is ranked into cand[(tile*Q + q)*k ..], the
// layout HZ_K_SEARCH_MERGE and HZ_K_SEARCH_RESCORE consume. Filtered only: `live` is required. span = 0: the launcher
// picks hz_search_pq_span(N, Q, M): about two workgroups per compute unit over the whole grid where the table lets one
// workgroup live on a compute unit (M >= 80), at most max(2, M / 16) below that. `f.s.queries` is not read
// by the scan (the merge's checks want it set). Refusals of either launcher (nothing is launched):
// -112 a null pointer (table kind: queries, codebook, lut; scan kind: corpus, queries, cand, out_score, out_id, lut);
// -113 D % M; -114 M % 16; -115 M outside 16..96; -116 D / M outside 1..64; -117 D > 2048; -118 ldc < M or ldc % 16;
// -119 N < 1; -120 Q outside 1..HZ_SEARCH_MAX_Q; -121 k outside 1..HZ_SEARCH_MAX_K; -122 corpus, queries, codebook or
// lut not 16-B, cand not 8-B or out_* / tags / filt / live not 4-B aligned; -123 a null live bitmap; -124 live_bytes
// below 4 * ceil(N / 32); -125 filt without tags; -126 cand_bytes below ntile * Q * k * 8; -127 lut_bytes below
// Q * M * 1024; -128 span < 0.
#define HZ_SEARCH_PQ_MAX_M 96
#define HZ_SEARCH_PQ_MAX_DSUB 64
typedef struct HzSearchPqLutParams {
  const float* queries;          // device fp32 [Q][D], 16-B aligned
  const float* codebook;         // device fp32 [M][256][D / M], 16-B aligned
  float* lut;                    // device fp32 [Q][M][256], 16-B aligned
  unsigned long long lut_bytes;  // bytes of `lut`, at least Q * M * 1024
  int D, M, Q, pad_;
} HzSearchPqLutParams;
typedef struct HzSearchPqParams {
  HzSearchFilterParams f;        // the filtered scan's block (live is required; corpus: byte rows, ldc in bytes)
  const float* lut;              // device fp32 [Q][M][256]: HZ_K_SEARCH_PQLUT's output
  unsigned long long lut_bytes;  // bytes of `lut`
  int M, span;                   // span: tiles a workgroup walks, 0 = the launcher's choice
} HzSearchPqParams;
int hz_search_pqlut_launch(const HzSearchPqLutParams* p, hipStream_t st);
int hz_search_pqscan_launch(const HzSearchPqParams* p, hipStream_t st);
// the span a launch with span = 0 takes for (N, Q, M) on the current device; 0 for a refused N, Q or M
int hz_search_pq_span(long long N, int Q, int M);
// nearest sub-centroids (HZ_K_SEARCH_PQASSIGN): what training and encoding a product quantiser spend
// their time in. rows: bf16 [N][ldr]; codebook: fp32 [M][256][dsub], dsub = D / M; codes: uint8 [N][ldc] (ldc in
// bytes) out; dist: fp32 [N][M] out, may be null.
// CONTRACT. For row r, sub-space m and centroid c
//   d(r, m, c) = the fp32 sum over j = 0 .. dsub-1, ascending, from +0, of t_j * t_j,
//   t_j        = float(rows[r][m*dsub + j]) - codebook[m][c][j],
// every subtraction, multiplication and addition a SEPARATE fp32 round-to-nearest operation: no FMA (numpy float32
// reproduces it bit for bit, hipzap.search.pq_assign_f32). codes[r][m] is the c with the smallest d, the lowest c
// among equal values: a strict d < best walking c upward from best = d(r, m, 0), so a NaN never displaces anything
// and an all-NaN column gives code 0. dist[r*M + m] holds the winner's d bits. Bytes M .. ldc-1 of a code row are not
// written; rows from N on are neither read nor written. The bits of a code and of a distance depend on the row's
// sub-vector and on codebook[m] only: not on N, the row's tile or position, the grid, or how the sub-spaces are
// grouped into workgroups (the kernel pads dsub to a multiple of 4 with zero columns: t = 0 - 0 = +0 and
// acc + +0 = acc for every acc the sum can hold, NaN included). Against the exact distance: all terms are
// non-negative, so |d^ - d| <= gamma(dsub + 2) * d, gamma(n) = n 2^-24 / (1 - n 2^-24), absent underflow.
// Grid (ceil(N / HZ_SEARCH_TILE), M / 16), HZ_SEARCH_TILE threads; thread t owns row t of the tile, the workgroup
// stages codebook[m] in LDS (dsub rounded up to a multiple of 4, KiB) for each of its 16 sub-spaces in turn.
// Refusals (nothing is launched): -129 a null rows, codebook or codes; -130 D % M; -131 M % 16; -132 M outside
// 16..96; -133 D / M outside 1..64; -134 D > 2048; -135 ldr < D or ldr % 8; -136 ldc < M or ldc % 16; -137 N < 1;
// -138 rows, codebook, codes or dist not 16-B aligned; -139 dist given with dist_bytes < N * M * 4.
typedef struct HzSearchPqAssignParams {
  const unsigned short* rows;     // device bf16 [N][ldr], 16-B aligned
  const float* codebook;          // device fp32 [M][256][D / M], 16-B aligned
  unsigned char* codes;           // device uint8 [N][ldc], 16-B aligned
  float* dist;                    // device fp32 [N][M], 16-B aligned, or null
  unsigned long long dist_bytes;  // bytes of `dist`, at least N * M * 4 when it is given
  long long N;
  int D, M;
  long long ldr, ldc;             // ldr in elements, ldc in bytes
} HzSearchPqAssignParams;
int hz_search_pqassign_launch(const HzSearchPqAssignParams* p, hipStream_t st);
// rescore (HZ_K_SEARCH_RESCORE): the second stage of a two-stage search. One workgroup per query
// scores the query against the R bf16 rows that `in_id` names (a merge's out_id of stage one; a slot is real
// iff (unsigned)id < (unsigned)N, every other value is an empty slot and nothing is loaded for it) and writes
// the best k of them under the order rule; the slots from the number of real candidates to k hold -inf / -1.
// The score bits of a real (q, r) are those of HZ_K_SEARCH_SCAN for the same query and the same bf16 row.
// Refusals: the scan's -2 (D, ldc), -3 (N), -4 (Q); -30 R outside 1..HZ_SEARCH_MAX_K, -31 k outside 1..R,
// -32 a null pointer, -33 rows or queries not 16-B aligned or in_id / out_* not 4-B aligned.
typedef struct HzSearchRescoreParams {
  const unsigned short* rows;    // bf16 [N][ldc], 16-B aligned rows; device memory or mapped pinned host memory
  const float* queries;          // fp32 [Q][D], 16-B aligned
  const int* in_id;              // int32 [Q][R], -1 in unused slots
  float* out_score;              // fp32 [Q][k]
  int* out_id;                   // int32 [Q][k]
  int N, D, Q, R, k, ldc;
} HzSearchRescoreParams;
int hz_search_rescore_launch(const HzSearchRescoreParams* p, hipStream_t st);
// list scan (HZ_K_SEARCH_LSCAN): the filtered scan over an indirect, per-query set of tiles of an
// IVF index. `f.s.N` stored rows are a whole number of tiles (padding rows are dead in `live`); `list_tiles` holds
// every tile id once, list l's tiles at [list_off[l], list_off[l + 1]); `rowid[r]` is the external id of stored row
// r. The grid is (P, Q): workgroup (j, q) scans the j-th tile of the lists probes[q][0 .. nprobe) in probe order
// against query q alone and writes its best k keys to cand[(j*Q + q)*k ..], the key's id field being
// ~rowid[row]; a workgroup past the probe set's tiles writes k zero keys. probes == NULL: every list -- P is
// N / HZ_SEARCH_TILE and workgroup j takes tile j. HZ_K_SEARCH_MERGE with N = P * HZ_SEARCH_TILE reduces the lists.
// The score bits of a passing (q, r) are those of HZ_K_SEARCH_SCAN for the same query and the same bf16 row.
// A probe id outside [0, nlist), offsets that are not 0 <= off[l] <= off[l + 1] <= N / HZ_SEARCH_TILE or a tile
// id outside [0, N / HZ_SEARCH_TILE) make the workgroup write zero keys; nothing is read through them.
// Refusals: the filtered scan's (its -7 is cand_bytes < P*Q*k*8 here); -40 nlist < 1; -41 nprobe outside
// 1..min(nlist, HZ_SEARCH_MAX_K) with probes; -42 P < 1, P * HZ_SEARCH_TILE >= 2^31, or P != N / HZ_SEARCH_TILE
// without probes; -43 N % HZ_SEARCH_TILE; -44 a null table; -45 a table or probes not 4-B aligned.
typedef struct HzSearchListParams {
  HzSearchFilterParams f;        // the filtered scan's block; f.s.cand holds [P][Q][k] keys
  const int* probes;             // device int32 [Q][nprobe] list ids (a merge's out_id), or NULL: every list
  const int* list_off;           // int32 [nlist + 1]: offsets into list_tiles
  const int* list_tiles;         // int32 [N / HZ_SEARCH_TILE]: the tile ids, list by list
  const int* rowid;              // int32 [N]: the external id of each stored row
  int nlist, nprobe, P, pad_;
} HzSearchListParams;
int hz_search_lscan_launch(const HzSearchListParams* p, hipStream_t st);
// quantised list scan (HZ_K_SEARCH_QLSCAN): the list scan over rows of OCP e4m3fn bytes with one fp32
// scale per stored row. `l.f.s.corpus` points at uint8 [N][ldc] (ldc in bytes, ldc % 16 == 0, D % 16 == 0,
// 16 <= D <= 2048). The score bits of a passing (q, r) are those of HZ_K_SEARCH_QSCAN for the same query, codes
// and scale; the codes and the scale of a dead or padding row are never loaded. Refusals: the byte rows' of the
// quantised launcher (-16 D % 16, -17 D < 16, -18 D > 2048, -19 ldc < D, -23 ldc % 16), every one of the list
// launcher, then -24 scales null and -25 scales not 4-B aligned.
typedef struct HzSearchQuantListParams {
  HzSearchListParams l;          // the list scan's block, unchanged
  const float* scales;           // fp32 [N] in stored order, 4-B aligned
} HzSearchQuantListParams;
int hz_search_qlscan_launch(const HzSearchQuantListParams* p, hipStream_t st);
// self scan (HZ_K_SEARCH_MSCAN): the queries are ROWS OF THE CORPUS, named by `qid`. The grid is
// (tile of HZ_SEARCH_TILE rows, block of HZ_SEARCH_SELF_QB queries); a workgroup reads its queries' rows by id and
// scores them against the tile's rows with v_mfma_f32_16x16x32_bf16, then writes per query the tile's best
// min(k, passing rows) keys, best first, then key 0, to cand[(tile*Q + q)*k ..]. Keys and their total order are
// the scan's. pass(q, r) = live(r) && !(skip_self && r == qid[q]); other rows with the query's bits stay and tie by
// id. A group of 16 rows with no live row is not loaded; a dead row of a mixed group is loaded and scores the
// sentinel. A qid outside [0, N) gives k zero keys for its query and nothing is read through it; the query's own
// live bit is not looked at (hz_index_neighbors refuses a deleted id). HZ_K_SEARCH_MERGEN reduces the lists.
// CONTRACT: every product of two bf16 values is exact in fp32; score(a, b) is the fp32 accumulator of the MFMAs
// over columns 0..31, 32..63, ... in that order, starting from +0, row a being the A operand and row b the B
// operand. Its bits depend on the D values of the two rows only: not on N, Q, k, the position of either row, the
// tile, or the other queries of the block. They are NOT the bits of HZ_K_SEARCH_SCAN for the widened query: that
// kind is one fmaf chain per lane and a butterfly, this one the matrix unit's sum, a different order of the same
// products. score(a, b) == score(b, a) is not promised.
// Refusals (nothing is launched): -50 corpus, qid, live or cand null; -51 D % 32; -52 D < 32; -53 D > 2048;
// -54 ldc < D or ldc % 8; -55 N < 1; -56 Q outside 1..HZ_SEARCH_SELF_MAX_Q (the grid's y limit of 65535 blocks);
// -57 k outside 1..HZ_SEARCH_MAX_K; -58 corpus not 16-B, cand not 8-B or qid / live not 4-B aligned;
// -59 live_bytes < 4 * ceil(N / 32); -60 cand_bytes < ntile * Q * k * 8.
#define HZ_SEARCH_SELF_QB 64
#define HZ_SEARCH_SELF_MAX_Q (65535 * HZ_SEARCH_SELF_QB)
typedef struct HzSearchSelfParams {
  const unsigned short* corpus;  // bf16 [N][ldc], 16-B aligned rows (ldc % 8 == 0), ldc >= D
  const int* qid;                // device int32 [Q]: the rows that are the queries
  const unsigned* live;          // 1 bit per row: bit r & 31 of word r >> 5 (required)
  unsigned long long* cand;      // scratch [ntile][Q][k] keys
  float* out_score;              // fp32 [Q][k]  (HZ_K_SEARCH_MERGEN only)
  int* out_id;                   // int32 [Q][k] (HZ_K_SEARCH_MERGEN only)
  unsigned long long live_bytes; // bytes of `live`, at least 4 * ceil(N / 32)
  unsigned long long cand_bytes; // bytes of `cand`, at least hz_search_self_scratch_bytes(N, Q, k)
  int N, D, Q, k, ldc;
  int ntile;                     // filled by the launchers: ceil(N / HZ_SEARCH_TILE)
  int skip_self, pad_;
} HzSearchSelfParams;
// ntile * Q * k * 8; 0 for a refused N, Q or k
unsigned long long hz_search_self_scratch_bytes(long long N, long long Q, int k);
int hz_search_mscan_launch(const HzSearchSelfParams* p, hipStream_t st);
// merge for any number of queries (HZ_K_SEARCH_MERGEN): search_merge_kernel, one workgroup per query over
// cand [ntile][Q][k] -> out_score / out_id [Q][k]. Reads cand, out_*, N, Q, k and cand_bytes of the block only.
// Refusals: -50 cand, out_score or out_id null; -55; -56; -57; -58 cand not 8-B or out_* not 4-B aligned; -60.
int hz_search_mergen_launch(const HzSearchSelfParams* p, hipStream_t st);
// batch scan (HZ_K_SEARCH_XSCAN): the self scan with an EXTERNAL A operand -- fp32 queries [Q][D] in
// place of `qid`, no skip_self. The grid, the tiles, the live bitmap's rules (a group of 16 rows with no live row is
// not loaded, a dead row of a mixed group is loaded and scores the sentinel), the candidate layout
// cand[(tile*Q + q)*k ..], the keys and their total order are HZ_K_SEARCH_MSCAN's. A query slot at or past Q loads
// nothing and writes nothing. HZ_K_SEARCH_MERGEN reduces the lists and takes THIS block as it stands: the two blocks
// have the same layout (`queries` where `qid` is, two unused ints where skip_self is) and the merge reads neither.
// THE SPLIT. A finite fp32 x is the exact sum of three bf16 values: h = the value of (bits(x) & 0xFFFF0000),
// m = the same truncation of x - h, l = (x - h) - m; both differences are exact in fp32 and l has at most 8
// significant bits. Then each of h, m, l whose exponent field is zero is replaced by a zero of its own sign, giving
// h', m', l' and the EFFECTIVE QUERY x' = h' + m' + l'. x' is a function of x alone (it does not depend on whether the
// matrix unit flushes subnormal inputs); x' == x unless a term is below 2^-126, which needs |x| < 2^-102.
// hipzap.search.split3 is the same function in numpy.
// CONTRACT. Every product of a term and a bf16 row value is exact in fp32. There is ONE accumulator per (q, r),
// starting from +0; per 32-column step s = 0, 1, ... (columns 32s .. 32s+31, ascending) it receives three MFMAs
// (v_mfma_f32_16x16x32_bf16, the query terms as the A operand) in the fixed order l', m', h'. The bits of score(q, r)
// depend on the D values of the query and of the row only: not on N, Q, k, the row's tile or position, the query's
// slot, or the other queries of the block. They are NOT the bits of HZ_K_SEARCH_SCAN (one fmaf chain per lane and a
// butterfly) or of HZ_K_SEARCH_MSCAN (one MFMA per step over a bf16 query). Error: the 3D additions inside and
// between the MFMAs are not documented as round-to-nearest, so against the exact sum_i x'_i r_i
//   |score - exact| <= beta(3D) * sum_i (|h'_i| + |m'_i| + |l'_i|) |r_i|,  beta(n) = n 2^-23 / (1 - n 2^-23).
// Refusals (nothing is launched; one code per case, the self scan's -50 .. -60 moved to -100 .. -110. They share the
// numbers -100 and -102 with hz_launch_kernel's "unknown kind" and "launcher not linked", which this kind never
// returns through a library that holds it): -100 corpus, queries, live or cand null; -101 D % 32; -102 D < 32;
// -103 D > 2048; -104 ldc < D or ldc % 8; -105 N < 1; -106 Q outside 1..HZ_SEARCH_SELF_MAX_Q; -107 k outside
// 1..HZ_SEARCH_MAX_K; -108 corpus not 16-B, cand not 8-B or live not 4-B aligned; -109 live_bytes < 4 * ceil(N / 32);
// -110 cand_bytes < ntile * Q * k * 8; -111 queries not 16-B aligned.
typedef struct HzSearchBatchParams {
  const unsigned short* corpus;  // bf16 [N][ldc], 16-B aligned rows (ldc % 8 == 0), ldc >= D
  const float* queries;          // device fp32 [Q][D], 16-B aligned
  const unsigned* live;          // 1 bit per row: bit r & 31 of word r >> 5 (required)
  unsigned long long* cand;      // scratch [ntile][Q][k] keys
  float* out_score;              // fp32 [Q][k]  (HZ_K_SEARCH_MERGEN only)
  int* out_id;                   // int32 [Q][k] (HZ_K_SEARCH_MERGEN only)
  unsigned long long live_bytes; // bytes of `live`, at least 4 * ceil(N / 32)
  unsigned long long cand_bytes; // bytes of `cand`, at least hz_search_self_scratch_bytes(N, Q, k)
  int N, D, Q, k, ldc;
  int ntile;                     // filled by the launchers: ceil(N / HZ_SEARCH_TILE)
  int pad_[2];                   // HzSearchSelfParams' skip_self and pad_: unused
} HzSearchBatchParams;
#ifdef __cplusplus
static_assert(sizeof(HzSearchBatchParams) == sizeof(HzSearchSelfParams) &&
                  offsetof(HzSearchBatchParams, cand) == offsetof(HzSearchSelfParams, cand) &&
                  offsetof(HzSearchBatchParams, out_id) == offsetof(HzSearchSelfParams, out_id) &&
                  offsetof(HzSearchBatchParams, cand_bytes) == offsetof(HzSearchSelfParams, cand_bytes) &&
                  offsetof(HzSearchBatchParams, ntile) == offsetof(HzSearchSelfParams, ntile),
              "HZ_K_SEARCH_MERGEN reads a batch block through HzSearchSelfParams");
#endif
int hz_search_xscan_launch(const HzSearchBatchParams* p, hipStream_t st);
// rescore for any number of queries (HZ_K_SEARCH_RESCOREN): search_rescore_kernel as it stands, one workgroup per
// query, behind a launcher that accepts Q up to HZ_SEARCH_SELF_MAX_Q -- as HZ_K_SEARCH_MERGEN stands to
// HZ_K_SEARCH_MERGE. The block, the score bits and every other refusal are HZ_K_SEARCH_RESCORE's (-4: Q outside
// 1..HZ_SEARCH_SELF_MAX_Q).
int hz_search_rescoren_launch(const HzSearchRescoreParams* p, hipStream_t st);
// nearest centroid of every row (HZ_K_SEARCH_ASSIGN): one workgroup of HZ_SEARCH_TILE threads per tile
// of HZ_SEARCH_TILE rows. The centroids are walked in blocks of HZ_SEARCH_ASSIGN_CB; a block's rows are the A operand
// of v_mfma_f32_16x16x32_bf16 and the tile's rows the B operand, both read with plain 16-byte loads (the fragment
// map and load schedule of HZ_K_SEARCH_MSCAN). Each row keeps one running best key (orderable(score) << 32) | ~c,
// the scan's total order: the highest score wins and, among centroids of equal score bits, the lowest index. After
// the last block the row's key is reduced over its four lanes and written: out_list[r] = c, out_score[r] = the score.
// No atomics, no scratch. `live` is ANY bitmap (the index passes live AND a sample mask): a row whose bit is 0
// writes out_list = -1, out_score = -inf; a group of 16 rows with no set bit is neither loaded nor multiplied; a
// dead row of a mixed group is loaded and its column of the product is dropped, so what it holds (NaN patterns
// included) reaches no other row. Rows from N on are not read and not written.
// CONTRACT: score(c, r) is the fp32 accumulator of the MFMAs over columns 0..31, 32..63, ... in that order,
// starting from +0, centroid c being the A operand and row r the B operand: HZ_K_SEARCH_MSCAN's statement. Its bits
// depend on the D values of the centroid and of the row only: not on N, C, the centroid's index or block, the row's
// tile or position, or the other bits of `live`. They are therefore HZ_K_SEARCH_MSCAN's bits for the same two
// D-vectors. Replays are bitwise equal. (out_score is +0.0 where the accumulator is -0.0, as in every search kind.)
// Refusals (nothing is launched): -61 corpus, cent, live, out_list or out_score null; -62 D % 32; -63 D < 32;
// -64 D > 2048; -65 ldc or ldk < D or not a multiple of 8; -66 N < 1; -67 C outside 1..HZ_SEARCH_ASSIGN_MAX_C;
// -68 corpus or cent not 16-B, live, out_list or out_score not 4-B aligned; -69 live_bytes < 4 * ceil(N / 32).
#define HZ_SEARCH_ASSIGN_CB 64
#define HZ_SEARCH_ASSIGN_MAX_C 65536  // IVF_MAX_LISTS of hipzap/search.py
typedef struct HzSearchAssignParams {
  const unsigned short* corpus;  // bf16 [N][ldc], 16-B aligned rows
  const unsigned short* cent;    // bf16 [C][ldk], 16-B aligned rows
  const unsigned* live;          // 1 bit per row: bit r & 31 of word r >> 5 (required)
  int* out_list;                 // int32 [N]
  float* out_score;              // fp32 [N]
  unsigned long long live_bytes; // bytes of `live`, at least 4 * ceil(N / 32)
  int N, D, C, ldc, ldk;
  int ntile;                     // filled by the launcher: ceil(N / HZ_SEARCH_TILE)
} HzSearchAssignParams;
int hz_search_assign_launch(const HzSearchAssignParams* p, hipStream_t st);
// the k-means update step (HZ_K_SEARCH_CMEAN): workgroup c replaces centroid c by the mean of the rows
// order[seg_off[c] .. seg_off[c + 1]). A member id outside [0, N) is skipped before any address is formed and does
// not count; a segment with no counted member, or whose bounds are not 0 <= seg_off[c] <= seg_off[c + 1] <= M, writes
// nothing (the centroid keeps its value). With `cosine` the mean is then divided by max(||mean||, 1e-12).
// cent32[c] (when not null) is the fp32 result, cent[c] its round-to-nearest-even bf16 bits.
// SUMMATION ORDER, a function of (member position, D) alone, no atomics: with nch = D / 8 and G = 256 / nch (integer
// division, 1..64), thread t < G * nch owns the 8 columns 8 * (t % nch) .. + 7 and the members at positions g, g + G,
// g + 2G, ... of the segment (g = t / nch), which it adds in that order to one fp32 sum per column starting from +0
// (a bf16 value widens exactly; a skipped member adds nothing). Column d's sum is then partial[0][d] + partial[1][d] +
// ... + partial[G - 1][d] in that order, divided by (float)count. ||mean||^2: thread t adds mean[d]^2 over d = t,
// t + 256, ... ascending from +0; the 64 lanes of a wave are summed by the xor butterfly 32, 16, .., 1 and the four
// waves' sums added in wave order. The bits of centroid c therefore depend on its own segment's rows and order only:
// not on C, on c or on the other segments.
// Refusals: -70 corpus, order, seg_off or cent null; -71 D % 32; -72 D < 32; -73 D > 2048; -74 ldc or ldk < D or
// not a multiple of 8; -75 N < 1; -76 C outside 1..HZ_SEARCH_ASSIGN_MAX_C; -77 M < 0; -78 corpus or cent not 16-B,
// order, seg_off or cent32 not 4-B aligned; -79 cosine not 0 or 1. seg_off and order live in device memory and are
// not checkable by the launcher: the kernel bounds every value it reads from them as stated above, and
// hz_index_cmean validates both on the host before the upload.
typedef struct HzSearchCmeanParams {
  const unsigned short* corpus;  // bf16 [N][ldc], 16-B aligned rows
  const int* order;              // device int32 [M]: the row ids of all members, cluster after cluster
  const int* seg_off;            // device int32 [C + 1]
  unsigned short* cent;          // bf16 [C][ldk], in and out
  float* cent32;                 // fp32 [C][D], out; may be null
  int N, D, C, M, ldc, ldk;
  int cosine, pad_;
} HzSearchCmeanParams;
int hz_search_cmean_launch(const HzSearchCmeanParams* p, hipStream_t st);
int hz_search_code_warm(void);

// an open .hzidx index (csrc/index.cpp): the bf16 row block in device memory plus `nctx` search contexts
// (stream, pinned query slot, device query buffer, candidate scratch, device and pinned result buffers).
// A context's program (H2D copy, scan, merge, two D2H copies) is captured per (Q, k) on first use.
// .hzidx: HzIndexHeader, the JSON header (json_len bytes), zero padding, the rows at data_off (4096-aligned);
// version 2 adds the JSON keys "capacity", "tags_off" and "live_off": two 4096-aligned blocks after the rows
// holding count u32 tags and the live bitmap (4 * ceil(count / 32) bytes). Version 1: all live, zero tags.
#define HZ_INDEX_MAGIC "HZIDX\0\0\1"
enum { HZ_INDEX_COSINE = 0, HZ_INDEX_IP = 1 };
typedef struct HzIndexHeader {
  char magic[8];
  uint32_t version, json_len;
  uint64_t data_off, count;
  uint32_t dim, metric;
} HzIndexHeader;
const char* hz_index_last_error(void);
void* hz_index_open(const char* path, int device, int nctx);  // nctx <= 0: 2
// out[8] = {count, dim, metric, contexts, tile rows, captured programs, device bytes, capacity}
int hz_index_describe(void* idx, uint64_t* out);
// queries fp32 [Q][dim] -> out_score [Q][k], out_id [Q][k]; blocks until the results are in host memory.
// One search at a time per context (a second caller of the same context waits).
int hz_index_search(void* idx, int ctx, const float* queries, int Q, int k, float* out_score, int* out_id);
void hz_index_close(void* idx);
// a live index. open2: rows, tags and the live bitmap are allocated for max(count, reserve_rows)
// rows rounded up to whole tiles. Ids are row positions, never reused. A mutation excludes every search: it
// holds all context mutexes and synchronises its copies before it returns.
void* hz_index_open2(const char* path, int device, int nctx, long long reserve_rows);
// out[8] = {capacity, live rows, tags present, filtered programs in use, the filtered programs' N, dtype, 0, 0};
// hz_index_describe's out[0] is the current count and out[7] the capacity
int hz_index_describe2(void* idx, uint64_t* out);
// filt: host [Q][2] u32 {mask, value} or NULL. A never-mutated index without filt runs scan + merge (N = count)
int hz_index_search_filtered(void* idx, int ctx, const float* queries, const unsigned* filt, int Q, int k,
                             float* out_score, int* out_id);
// append n bf16 rows (finite values: the caller checks) at ids [count, count + n); grows by doubling
int hz_index_add(void* idx, const unsigned short* rows_bf16, long long n, const unsigned* tags_or_null, long long* first_id_out);
int hz_index_delete(void* idx, const int* ids, long long n, long long* newly_deleted_out);  // -20: an id outside [0, count)
int hz_index_set_tags(void* idx, const int* ids, const unsigned* tags, long long n);
// the first n rows / tag words / ceil(n / 32) live words to host memory (any pointer may be NULL)
int hz_index_read_state(void* idx, unsigned short* rows_out, unsigned* tags_out, unsigned* live_out, long long n);
// an fp8 index (a version-3 .hzidx): rows are [count][dim] e4m3fn bytes, and "scales_off" of the
// JSON header names a 4096-aligned block of count fp32 scales after them (tags and bitmap, when present, follow).
// hz_index_open2 opens it; every search replays H2D, HZ_K_SEARCH_QSCAN, merge, two D2H. hz_index_describe2's
// out[5] is the dtype (0 bf16, 1 fp8_e4m3). The _q calls are hz_index_add / hz_index_read_state for such an
// index; each form refuses (-26, hz_index_last_error names both dtypes) an index of the other dtype.
int hz_index_add_q(void* idx, const unsigned char* codes, const float* scales, long long n, const unsigned* tags_or_null,
                   long long* first_id_out);
int hz_index_read_state_q(void* idx, unsigned char* codes_out, float* scales_out, unsigned* tags_out, unsigned* live_out,
                          long long n);
// a two-stage index (a version-4 .hzidx): version 3 plus the JSON keys "rescore": "bf16" and
// "rescore_off", a 4096-aligned block of [count][dim] bf16 rows after every version-3 block -- the rows a bf16
// index of the same vectors holds. open3 opens any version; for version 4 the bf16 rows go to device memory
// (rescore_host = 0; open / open2 do this) or to pinned host memory that the rescore kernel reads through its
// mapped address, which leaves the index at an fp8 index's device bytes. describe2's out[6] is 1 for an index
// with rescore rows and out[7] their placement (0 device, 1 host).
void* hz_index_open3(const char* path, int device, int nctx, long long reserve_rows, int rescore_host);
// refine = 0: hz_index_search_filtered. refine = R, k <= R <= HZ_SEARCH_MAX_K: the fp8 scan and merge at k = R,
// then HZ_K_SEARCH_RESCORE of those R ids against the bf16 rows -> the best k. -27: the index has no rescore
// rows; -28: R outside k..HZ_SEARCH_MAX_K (hz_index_last_error says which).
int hz_index_search2(void* idx, int ctx, const float* queries, const unsigned* filt, int Q, int k, int refine,
                     float* out_score, int* out_id);
// append rows to a two-stage index: codes, scales and bf16 rows together, so a row is fully present or absent.
// -29 (with a message naming the right call): hz_index_add_q on a two-stage index, or this call on any other.
int hz_index_add_qr(void* idx, const unsigned char* codes, const float* scales, const unsigned short* rows_bf16,
                    long long n, const unsigned* tags_or_null, long long* first_id_out);
int hz_index_read_rescore(void* idx, unsigned short* rows_out, long long n);  // the first n bf16 rescore rows
// an IVF index (a version-5 .hzidx): version 2 whose rows, tags and live bitmap are stored list by
// list, every list on a tile boundary (capacity = tiles * HZ_SEARCH_TILE stored rows, padding rows dead), plus
// the JSON block "ivf": nlist, nprobe, seed, iters and the offsets of four 4096-aligned blocks -- centroids_off
// (bf16 [nlist][dim]), list_off_off (int32 [nlist + 1]), list_tiles_off (int32 [tiles]) and rowid_off (int32
// [capacity], -1 on padding). open3 opens it (and refuses inconsistent tables); ids are the external ids.
// search3: nprobe = 0 scans every list (no coarse stage); 1 <= nprobe < nlist replays H2D, scan + merge over the
// centroids at k = nprobe, HZ_K_SEARCH_LSCAN over those lists with P = the tiles of the nprobe largest lists,
// merge, two D2H. -34: nprobe on an index without lists, nprobe outside 0..min(nlist, HZ_SEARCH_MAX_K), refine
// on an IVF index, or hz_index_add on one (hz_index_last_error says which). On any other index search3 with
// nprobe = 0 is search2.
int hz_index_search3(void* idx, int ctx, const float* queries, const unsigned* filt, int Q, int k, int refine,
                     int nprobe, float* out_score, int* out_id);
// the coarse stage alone: the nprobe best lists of each query, best first -> out_list int32 [Q][nprobe]
int hz_index_probes(void* idx, int ctx, const float* queries, int Q, int nprobe, int* out_list);
// An fp8 IVF index (a version-6 or version-7 .hzidx): version 5's layout over version 3's rows --
// e4m3 codes [capacity][dim] and "scales_off" fp32 [capacity], both in stored order (padding: code 0, scale 1, dead).
// Its programs replace HZ_K_SEARCH_LSCAN by HZ_K_SEARCH_QLSCAN. Version 7 adds "rescore": "bf16" / "rescore_off":
// bf16 [count][dim] in EXTERNAL-ID order, the last block (device or pinned host memory per open3's rescore_host).
// search3 with refine = R on it: list scan and merge at k = R, then HZ_K_SEARCH_RESCORE over rows[id] with
// N = count. -34 stays the answer to refine on an IVF index without rescore rows. hz_index_read_state_q returns the
// stored rows, hz_index_read_rescore up to count rows by id. Rows are never added (-34).
// out[8] = {1 for an IVF index, nlist, default nprobe, tiles, external count, the file's version, 0, 0}
int hz_index_describe3(void* idx, uint64_t* out);
// A binary index (a version-8 or version-9 .hzidx): version 3's rule set over sign-bit rows --
// "dtype": "bin_sign", the row block uint32 [count][dim / 32] (dim % 128 == 0, 128 <= dim <= 2048), no scales block,
// "capacity" / "tags_off" / "live_off" present exactly when version 3 would have them. Version 9 adds "rescore":
// "bf16" / "rescore_off" as version 4 does. open3 opens both (either rescore placement); every search replays H2D,
// HZ_K_SEARCH_BSCAN, merge, two D2H, and with refine = R the scan and merge at k = R, then HZ_K_SEARCH_RESCORE:
// version 4's programs with the binary scan in place of the fp8 scan, under the same key and invalidation rules.
// describe2's out[5] is 2. The _b calls are hz_index_add / hz_index_read_state for such an index (-26 on any other
// dtype, and from the other forms on this one); hz_index_add_br takes the words and the bf16 rows together, live
// bits set last (-29, naming the right call: add_b on a version-9 index, add_br on a version-8 one). nprobe, probes
// (-34), neighbors (-35), assign and cmean (-38) refuse it by name: "a bin_sign index of version 8".
int hz_index_add_b(void* idx, const unsigned* words, long long n, const unsigned* tags_or_null, long long* first_id_out);
int hz_index_add_br(void* idx, const unsigned* words, const unsigned short* rows_bf16, long long n,
                    const unsigned* tags_or_null, long long* first_id_out);
int hz_index_read_state_b(void* idx, unsigned* words_out, unsigned* tags_out, unsigned* live_out, long long n);
// A product-quantised index (a version-10 or version-11 .hzidx): version 3's rule set over pq8 rows --
// "dtype": "pq8", the JSON block "pq": {"m": M, "ksub": 256, "dsub": dim / M, "codebook_off": ...}, the row block uint8
// [count][M], the codebook fp32 [M][256][dsub] in a 4096-aligned block after it, no scales block, "capacity" /
// "tags_off" / "live_off" present exactly when version 3 would have them. Version 11 adds "rescore": "bf16" /
// "rescore_off" as version 4 does, the last block. open3 opens both (either rescore placement), uploads the codebook
// and gives every context a table scratch [HZ_SEARCH_MAX_Q][M][256] fp32; every search replays H2D,
// HZ_K_SEARCH_PQLUT, HZ_K_SEARCH_PQSCAN, merge, two D2H, and with refine = R the scan and merge at k = R, then
// HZ_K_SEARCH_RESCORE: version 4's programs under the same key and invalidation rules. describe2's out[5] is 3;
// describe4 reports M, dsub and the codebook's bytes. The _p calls are hz_index_add / hz_index_read_state for such an
// index (-26 on any other dtype, and from the other forms on this one): the codes are encoded by the caller against
// the index's codebook (hz_index_read_codebook); hz_index_add_pr takes the codes and the bf16 rows together (-29,
// naming the right call: add_p on a version-11 index, add_pr on a version-10 one). nprobe, probes (-34), neighbors
// (-35), assign and cmean (-38) and search_batch (-44) refuse it by name: "a pq8 index of version 10".
int hz_index_add_p(void* idx, const unsigned char* codes, long long n, const unsigned* tags_or_null, long long* first_id_out);
int hz_index_add_pr(void* idx, const unsigned char* codes, const unsigned short* rows_bf16, long long n,
                    const unsigned* tags_or_null, long long* first_id_out);
int hz_index_read_state_p(void* idx, unsigned char* codes_out, unsigned* tags_out, unsigned* live_out, long long n);
int hz_index_read_codebook(void* idx, float* codebook_out);  // fp32 [M][256][dsub]; -26 on any other dtype
// out[8] = {M, dsub, codebook bytes, table scratch bytes per context, the span of a Q = 1 scan, 0, 0, 0}; zeros
// unless the index holds pq8 rows
int hz_index_describe4(void* idx, uint64_t* out);
// neighbours of stored rows (a plain bf16 index, versions 1 and 2, dim % 32 == 0): the k nearest live
// rows of each of the n rows `ids` names, the row itself excluded iff skip_self -> out_score fp32 [n][k], out_id
// int32 [n][k], -inf / -1 past the live rows. Replays H2D of the ids, HZ_K_SEARCH_MSCAN, HZ_K_SEARCH_MERGEN, two
// D2H; captured per (n, k, skip_self). One call takes at most HZ_INDEX_SELF_MAX_Q ids (the caller splits above it):
// the candidate scratch of a context, allocated on first use and grown on demand, is ceil(capacity /
// HZ_SEARCH_TILE) * n * k * 8 bytes, so at most tiles * HZ_INDEX_SELF_MAX_Q * HZ_SEARCH_MAX_K * 8.
// -4: n outside 1..the maximum; -5: k; -20: an id outside [0, count); -35: an fp8 or an IVF index; -36: dim % 32;
// -37: a deleted id (hz_index_last_error names the value in each case).
#define HZ_INDEX_SELF_MAX_Q 1024
int hz_index_neighbors(void* idx, int ctx, const int* ids, int n, int k, int skip_self, float* out_score, int* out_id);
// the ids one hz_index_neighbors call (and the queries one hz_index_search_batch call) takes; set in
// 1..HZ_INDEX_SELF_MAX_Q lowers or restores it first (0: only read)
int hz_index_neighbors_max(void* idx, int set);
// bulk search (a plain bf16 index, versions 1 and 2, dim % 32 == 0): Q external fp32 queries at once
// -> out_score fp32 [Q][k], out_id int32 [Q][k], -inf / -1 past the live rows, and out_stage1_last fp32 [Q]. Replays
// H2D of the queries, HZ_K_SEARCH_XSCAN at k = R, HZ_K_SEARCH_MERGEN (the R best rows of each query by the batch
// scan's score), HZ_K_SEARCH_RESCOREN of those ids against the index's own rows (R -> k, the bits and the order of
// hz_index_search) and three D2H; captured per (Q, k, R) under hz_index_neighbors' program rules. out_stage1_last[q]
// is the batch scan's score of query q's R-th candidate, -inf when fewer than R rows passed: all the host needs to
// prove that no row outside the candidates can belong to the answer (hipzap.search.batch_certain). One call takes
// at most hz_index_neighbors_max queries (HZ_INDEX_SELF_MAX_Q unless lowered; the caller splits above it); a
// context's buffers for it are allocated on first use and the candidate scratch, shared with hz_index_neighbors and
// grown on demand, is ceil(capacity / HZ_SEARCH_TILE) * Q * R * 8 bytes.
// -4: Q outside 1..the maximum; -5: k; -28: R outside k..HZ_SEARCH_MAX_K; -44: an fp8, a binary or an IVF index;
// -45: dim % 32 (hz_index_last_error names the value in each case).
int hz_index_search_batch(void* idx, int ctx, const float* queries, int Q, int k, int R, float* out_score, int* out_id,
                          float* out_stage1_last);
// clustering (a plain bf16 index, versions 1 and 2, dim % 32 == 0). Batch jobs: plain launches on the
// context's stream under its mutex, no captured program; a context's buffers for them are allocated on first use
// and grown on demand (a call that needs no more than an earlier one allocates nothing).
// hz_index_assign: the nearest of the C centroids `cent_bits` (bf16 [C][dim]) for every row -> out_list int32
// [count], out_score fp32 [count]. `mask_words` (null: every row) holds one bit per row, ceil(count / 32) words; a
// row takes part iff it is live and its mask bit is set, every other row gets -1 / -inf. Uploads the centroids and
// live AND mask, launches HZ_K_SEARCH_ASSIGN over the filtered programs' N, copies both arrays back.
// hz_index_cmean: centroid c becomes the mean of the rows order[seg_off[c] .. seg_off[c + 1]) (divided by its norm on
// a cosine index), an empty segment keeps its value: HZ_K_SEARCH_CMEAN over `cent_bits_inout`; `cent32_out` (may be
// null) receives the fp32 values [C][dim], untouched where the segment is empty.
// -38: an fp8 or an IVF index; -39: dim % 32; -40: C outside 1..HZ_SEARCH_ASSIGN_MAX_C; -41: M outside [0, 2^31);
// -42: seg_off not 0 = seg_off[0] <= ... <= seg_off[C] = M; -43: a member id outside [0, count)
// (hz_index_last_error names the value in each case).
int hz_index_assign(void* idx, int ctx, const unsigned short* cent_bits, int C, const unsigned* mask_words, int* out_list,
                    float* out_score);
int hz_index_cmean(void* idx, int ctx, const int* order, long long M, const int* seg_off, int C,
                   unsigned short* cent_bits_inout, float* cent32_out);
// hz_pq_encode: HZ_K_SEARCH_PQASSIGN over n host rows (bf16 [n][dim]) against `codebook` (host fp32
// [m][256][dim / m]) on `device` -> codes_out uint8 [n][m], dist_out_or_null fp32 [n][m]. Not tied to an open index
// (a file is usually being built when it runs). A plain batch job on a stream of its own, no captured program: the
// codebook is uploaded once, the rows go through device buffers `chunk_rows` at a time (0: a default; any other
// value is honoured, so a chunk edge can sit anywhere) and each chunk's codes (and distances) are copied back.
// A refused shape returns the launcher's code (-129 .. -137); -140: hipSetDevice, an allocation, a copy or the
// stream failed, -141: chunk_rows < 0 (hz_index_last_error says which call and why).
int hz_pq_encode(int device, const unsigned short* rows_bf16, long long n, int dim, int m, const float* codebook,
                 long long chunk_rows, unsigned char* codes_out, float* dist_out_or_null);

// row softmax: out[r][i] = exp(s*x[r][i] + mask[i] - m_r) / sum_i(...), i < D
typedef struct HzSoftmaxParams {
  const void* x;       // [rows][ldx] fp32 (x_bf16 = 0) or bf16
  const float* mask;   // optional additive [D] mask
  float* out;          // [rows][ldo] fp32
  int rows, D, ldx, ldo, x_bf16;
  float scale;
} HzSoftmaxParams;
int hz_softmax_launch(const HzSoftmaxParams* p, hipStream_t st);

// ---- fused ResNet stages (csrc/block.hip; bs=1 dispatch count) ----
// stem: image -> normalise -> 7x7/2 conv (packed like conv1: cin_pad 8, 13 k-steps) + bias + ReLU ->
// 3x3/2 max-pool pad 1, channel-blocked output; one launch instead of preprocess + conv + maxpool
typedef struct HzStemParams {
  const void* src;            // uint8 NHWC [N][H][W][3] (mode 1), fp32 NCHW [N][3][H][W] (mode 0), or bf16
                              // NHWC [N][H][W][8] already normalised (mode 2: after the preprocess kernel)
  const unsigned short* w;    // fragment-major [4][13][64][8], k = (r*7 + s)*8 + c
  const float* bias;          // [64]
  unsigned short* out;        // [N][2][PH][PW][32]
  int N, H, W, mode;
  int SH, SW, PH, PW;         // stem output / pooled sizes
  int norm, pad_;             // norm: (x - mean) * inv_std (mode 1 scales bytes by 1/255 first)
  float mean[4], inv_std[4];
} HzStemParams;
// one bottleneck block at layer1 geometry (Cmid 64, Cout 256, stride 1): conv1 1x1 -> conv2 3x3 ->
// conv3 1x1 + residual (identity when wd == NULL, else the 1x1 downsample) + ReLU, each workgroup an
// 8x8 output tile recomputing its conv1 halo; H, W multiples of 8
typedef struct HzBneckParams {
  const unsigned short* x;    // [N][Cin/32][H][W][32]
  const unsigned short* w1;   // packed as the per-conv kernels (fragment-major, K order (r, s, c))
  const float* b1;
  const unsigned short* w2;
  const float* b2;
  const unsigned short* w3;
  const float* b3;
  const unsigned short* wd;   // downsample (layer1: Cin 64; layer2: Cin 256, stride 2) or NULL (identity)
  const float* bd;
  unsigned short* out;        // [N][Cout/32][H][W][32]
  int N, H, W, Cin, Cmid, Cout;  // H, W: the block's OUTPUT size (the input is 2H x 2W for the
                                 //   stride-2 first block of layer2)
  int tile_h;                 // layer1 output tile rows: 8 (default when 0) or 4 (twice the workgroups)
  int imgs;                   // layer2 images per workgroup: 0 auto (2 at an even N >= 8), 1, 2
} HzBneckParams;
// ResNet 1x1 -> 1x1 seam at 14x14 / 7x7 (layer3 / layer4, bs=1): conv3 of block i (1x1 CM -> 4CM,
// + residual + ReLU) and the K-split conv1 of block i+1 (1x1 4CM -> CM) in ONE launch. A workgroup
// owns (pixel tile <= 32, slice of cs of the 4CM channels): it computes that slice of y = relu(W3 t2
// + b3 + res) over the full K, stores it, and adds W1[:, slice] . y_slice into the fp32 accumulator z
// (no-return float atomics; z was set to conv1's bias by the launch before, see HzConvParams.zinit);
// block i+1's 3x3 conv reads z with ReLU at its operand load (HzConvParams.x_f32). No workgroup
// waits for another: the conv1 reduction happens in the memory-side atomic units.
typedef struct HzSeamParams {
  const unsigned short* t2;   // conv3 input [N][CM/32][HW][32] bf16
  const unsigned short* w3;   // conv3 weights, packed as the per-conv kernels ([4CM/16][CM/32][64][8])
  const float* b3;            // [4CM]
  const unsigned short* res;  // residual [N][4CM/32][HW][32]
  unsigned short* y;          // block output [N][4CM/32][HW][32]
  const unsigned short* w1;   // next conv1 weights [CM/16][4CM/32][64][8]
  float* z;                   // next conv1 accumulator [N][CM/32][HW][32] fp32, preset to its bias
  int N, HW, CM, cs;          // cs: slice width (64 or 128)
  int tiles, t2_f32;          // tiles: pixel tiles per image (launcher: ceil(HW / 32)); t2_f32: t2 is the
                              //   fp32 accumulator of a K-split 3x3 conv (ReLU applied at the load)
  float* zinit;               // or NULL: afterwards filled with zbias per channel ([N][z_C/32][z_HW][32]):
  const float* zbias;         //   the next K-split 3x3 conv's accumulator
  int z_C, z_HW;
  int tail, pad_;             // tail: the last block -- conv3 + global average pool, no conv1 half (w1, z
                              //   unused): fp32 [N][4CM] means into y's buffer (HW <= 64, CM 512)
  int cn;                     // conv1 outputs (0: CM); 512 at CM 256 = the layer3 -> layer4 seam
  int ds;                     // 1: the residual is the stride-2 1x1 downsample of xd (res unused):
  const unsigned short* xd;   //   [N][2CM/32][xd_H][xd_W][32] bf16, the stage input
  const unsigned short* wd;   //   packed like the per-conv kernels ([4CM/16][2CM/32][64][8])
  const float* bd;            //   [4CM]
  int xd_H, xd_W;
} HzSeamParams;
// K-split 3x3 conv (pad 1, stride 1 at <= 14 x 14 or stride 2 from <= 28 x 28) into an fp32
// accumulator (block.hip kconv_kernel):
// a workgroup owns (image, 32 output channels, a slice of ck input channels): it stages that slice of
// the whole image (+ zero halo) in LDS once -- bf16, or fp32 with the ReLU applied (x_f32: a seam's
// conv1 sum) -- multiplies all 9 taps from LDS (mfma 32x32x16, pixels on the A rows) and adds its
// partial into `out` by float atomics (out preset to the conv's bias by the launch before; the
// consumer applies the ReLU when it loads out). Each input byte is read from L2 once per workgroup
// instead of once per tap; the weight stream is split over C/ck workgroups per channel tile.
typedef struct HzKconvParams {
  const void* x;              // [N][C/32][H][W][32] fp32 (x_f32) or bf16
  const unsigned short* w;    // packed as the per-conv kernels: [Cout/16][9C/32][64][8], k = (r*3 + s)*C + c
  float* out;                 // [N][Cout/32][H][W][32] fp32, preset to the bias
  float* zinit;               // or NULL: filled with zbias per channel afterwards, as HzConvParams.zinit
  const float* zbias;
  int z_C, z_HW;
  int N, H, W, C, Cout, x_f32;  // H, W: the INPUT size (the output is H/stride x W/stride)
  int ck, stride;             // input channels per workgroup: 32, 64 or 128; stride 1 or 2
  // optional second job of the launch (dso != NULL): the block's stride-2 1x1 downsample, in its
  // own workgroups (32 output channels x <= 64 output pixels, full K): dso = dsw dsx(2y, 2x) + dsb
  const unsigned short* dsx;  // [N][ds_C/32][ds_H][ds_W][32] bf16
  const unsigned short* dsw;  // packed [ds_Cout/16][ds_C/32][64][8]
  const float* dsb;           // [ds_Cout]
  unsigned short* dso;        // [N][ds_Cout/32][ds_H/2][ds_W/2][32] bf16
  int ds_C, ds_Cout, ds_H, ds_W;
} HzKconvParams;
int hz_stem_launch(const HzStemParams* p, hipStream_t st);
int hz_bneck_launch(const HzBneckParams* p, hipStream_t st);
int hz_seam_launch(const HzSeamParams* p, hipStream_t st);
int hz_kconv_launch(const HzKconvParams* p, hipStream_t st);
int hz_block_code_warm(void);

// ---- the kernel table: every launch a program can hold ----
// argument records of the launchers that take scalars or a cfg beside their parameter struct
typedef struct HzConvOp {
  HzConvParams p;
  int cfg, pad_;
} HzConvOp;
typedef struct HzConv2Op {
  HzConvParams a, b;
  int cfg, pad_;
} HzConv2Op;
typedef struct HzAvgpoolArgs {
  const unsigned short* x;
  unsigned short* out;
  int N, HW, C, blocked;
} HzAvgpoolArgs;
typedef struct HzPreprocessArgs {
  const void* src;
  unsigned short* dst;
  const float* mean;
  const float* inv_std;
  int N, Cin, H, W, Cpad, mode;
} HzPreprocessArgs;
typedef struct HzStepBumpArgs {
  int* step;
  int n, pad_;
} HzStepBumpArgs;
typedef struct HzDiagArgs {  // hz_diag_launch (csrc/diag.hip)
  int kind, blocks, threads, pad_;
  void* a;
  void* b;
  long bytes;
} HzDiagArgs;
// translation units holding device code (hz_plan_open warms the ones a plan's kernels live in)
enum { HZ_UNIT_CONV = 1, HZ_UNIT_VISION = 2, HZ_UNIT_GEMM = 4, HZ_UNIT_TRANSFORMER = 8, HZ_UNIT_FP8 = 16,
       HZ_UNIT_PACK = 32, HZ_UNIT_BLOCK = 64, HZ_UNIT_LSTM = 128, HZ_UNIT_LMBATCH = 256, HZ_UNIT_DIAG = 512,
       HZ_UNIT_SEARCH = 1024 };
// X(NAME, value, parameter struct, launcher, code unit): the ONE list of kinds. A launcher is
// `int f(const Params*, hipStream_t)`; the *_op launchers are the adapters in runtime.cpp that unpack
// an argument record. hz_launch_kernel, hz_kernel_param_size, hz_kernel_name, hz_kernel_code_unit and
// the struct sizes in hz_abi_version are generated from it; hipzap/_native.py KINDS mirrors the values
// (tests/test_kinds_cpu.py compares the two). Values are never reused: 17 (the persistent
// dependent-conv chain) was removed in round 5, measured negative in round 3 (profiles/r3_chain).
#define HZ_KERNELS(X)                                                     \
  X(CONV, 1, HzConvOp, hz_conv_op, CONV)                                  \
  X(LAYERNORM, 2, HzLayerNormParams, hz_layernorm_launch, TRANSFORMER)    \
  X(EMBED, 3, HzEmbedParams, hz_embed_ln_launch, TRANSFORMER)             \
  X(ATTENTION, 4, HzAttentionParams, hz_attention_launch, TRANSFORMER)    \
  X(VIT_TOKENS, 5, HzVitTokensParams, hz_vit_tokens_launch, TRANSFORMER)  \
  X(LSTM, 6, HzLstmParams, hz_lstm_cell_launch, LSTM)                     \
  X(DECODER, 7, HzDecoderParams, hz_decoder_launch, LSTM)                 \
  X(SAMPLER, 8, HzSamplerParams, hz_sampler_launch, LSTM)                 \
  X(MAXPOOL, 9, HzPoolParams, hz_maxpool_launch, VISION)                  \
  X(QUANT, 10, HzQuantParams, hz_quant_launch, FP8)                       \
  X(GEMM_FP8, 11, HzGemmFp8Params, hz_gemm_fp8_launch, FP8)               \
  X(SOFTMAX, 12, HzSoftmaxParams, hz_softmax_launch, TRANSFORMER)         \
  X(POOL_FC, 13, HzPoolFcParams, hz_pool_fc_launch, VISION)               \
  X(LMB_LAYER, 14, HzLmbLayerParams, hz_lmb_layer_launch, LMBATCH)        \
  X(LMB_DEC, 15, HzLmbDecParams, hz_lmb_dec_launch, LMBATCH)              \
  X(LMB_ADMIT, 16, HzLmbAdmitParams, hz_lmb_admit_launch, LMBATCH)        \
  X(STEM, 18, HzStemParams, hz_stem_launch, BLOCK)                        \
  X(BNECK, 19, HzBneckParams, hz_bneck_launch, BLOCK)                     \
  X(SEAM, 20, HzSeamParams, hz_seam_launch, BLOCK)                        \
  X(KCONV, 21, HzKconvParams, hz_kconv_launch, BLOCK)                     \
  X(QKVATT, 22, HzQkvAttParams, hz_qkvatt_launch, TRANSFORMER)            \
  X(CONV2, 23, HzConv2Op, hz_conv2_op, CONV)                              \
  X(AVGPOOL, 24, HzAvgpoolArgs, hz_avgpool_op, VISION)                    \
  X(PREPROCESS, 25, HzPreprocessArgs, hz_preprocess_op, VISION)           \
  X(STEP_BUMP, 26, HzStepBumpArgs, hz_step_bump_op, LSTM)                 \
  X(DIAG, 27, HzDiagArgs, hz_diag_op, DIAG)                               \
  X(RESIZE_PREPROCESS, 28, HzResizeParams, hz_resize_preprocess_op, VISION) \
  X(POOL_EMBED, 29, HzPoolEmbedParams, hz_pool_embed_op, TRANSFORMER)     \
  X(RESIZE_PATCHIFY, 30, HzResizeParams, hz_resize_patchify_op, VISION)   \
  X(SEARCH_SCAN, 31, HzSearchParams, hz_search_scan_op, SEARCH)           \
  X(SEARCH_MERGE, 32, HzSearchParams, hz_search_merge_op, SEARCH)         \
  X(SEARCH_FSCAN, 33, HzSearchFilterParams, hz_search_fscan_op, SEARCH)   \
  X(SEARCH_QSCAN, 34, HzSearchQuantParams, hz_search_qscan_op, SEARCH)   \
  X(SEARCH_RESCORE, 35, HzSearchRescoreParams, hz_search_rescore_op, SEARCH) \
  X(SEARCH_LSCAN, 36, HzSearchListParams, hz_search_lscan_op, SEARCH)     \
  X(SEARCH_QLSCAN, 37, HzSearchQuantListParams, hz_search_qlscan_op, SEARCH) \
  X(POOL_NORM, 38, HzPoolNormParams, hz_pool_norm_op, VISION)               \
  X(SEARCH_MSCAN, 39, HzSearchSelfParams, hz_search_mscan_op, SEARCH)     \
  X(SEARCH_MERGEN, 40, HzSearchSelfParams, hz_search_mergen_op, SEARCH)   \
  X(SEARCH_ASSIGN, 41, HzSearchAssignParams, hz_search_assign_op, SEARCH) \
  X(SEARCH_CMEAN, 42, HzSearchCmeanParams, hz_search_cmean_op, SEARCH)   \
  X(SEARCH_BSCAN, 43, HzSearchBinParams, hz_search_bscan_op, SEARCH)     \
  X(SEARCH_XSCAN, 44, HzSearchBatchParams, hz_search_xscan_op, SEARCH)    \
  X(SEARCH_RESCOREN, 45, HzSearchRescoreParams, hz_search_rescoren_op, SEARCH) \
  X(SEARCH_PQLUT, 46, HzSearchPqLutParams, hz_search_pqlut_op, SEARCH)    \
  X(SEARCH_PQSCAN, 47, HzSearchPqParams, hz_search_pqscan_op, SEARCH)  \
  X(SEARCH_PQASSIGN, 48, HzSearchPqAssignParams, hz_search_pqassign_op, SEARCH)
#define HZ_KERNEL_ENUM(NAME, value, T, fn, unit) HZ_K_##NAME = value,
enum { HZ_KERNELS(HZ_KERNEL_ENUM) };
#undef HZ_KERNEL_ENUM
int hz_launch_kernel(int kind, const void* params, hipStream_t st);
int hz_experiments(void);  // 1: built with HZ_EXPERIMENTS (measured-negative kernel variants)
size_t hz_kernel_param_size(int kind);  // 0: unknown kind
const char* hz_kernel_name(int kind);   // "HZ_K_<NAME>", NULL: unknown kind
unsigned hz_kernel_code_unit(int kind); // HZ_UNIT_* of the kind's device code, 0: unknown kind

// ---- runtime: static op programs, graph capture / replay ----
HzProgram hz_prog_create(void);
void hz_prog_destroy(HzProgram p);
int hz_prog_num_ops(HzProgram p);
// a launch of `kind`: the parameter block (at least hz_kernel_param_size(kind) bytes) is copied
int hz_prog_add_kernel(HzProgram p, int kind, const void* params, size_t size, int slot);
int hz_prog_add_memcpy(HzProgram p, void* dst, const void* src, size_t bytes, int slot);  // any direction (UVA)
int hz_prog_add_fork(HzProgram p, int slot);   // side stream `slot` waits for main
int hz_prog_add_join(HzProgram p, int slot);   // main waits for side stream `slot`
int hz_prog_run(HzProgram p, hipStream_t st);  // eager launch of every op
int hz_prog_capture(HzProgram p, hipStream_t st);
int hz_prog_replay(HzProgram p, hipStream_t st);
int hz_prog_is_captured(HzProgram p);
// make the side streams / fork events a run needs (before a lazy capture races a replay)
int hz_prog_prepare(HzProgram p);
int hz_prog_replay_n(HzProgram p, hipStream_t st, int n);  // n back-to-back replays, no sync
// replay `n` programs round-robin on `n` streams `iters` times from C++ and synchronize;
// returns elapsed microseconds (host wall, includes the final sync) or negative on error.
double hz_prog_bench(HzProgram* progs, hipStream_t* streams, int n, int iters);
int hz_prog_bench2(HzProgram* progs, hipStream_t* streams, int n, int iters, int threads, double* out);
// closed-loop serving benchmark (one host thread per context; per-request latency in lat_us[n*iters])
int hz_serve_bench(HzProgram* progs, hipStream_t* streams, void** in_dst, void** in_src, uint64_t in_bytes,
                   void** out_src, void** out_dst, uint64_t out_bytes, int n, int iters, double* lat_us,
                   double* wall_us);
// ---- request slots: a context's INPUT buffer, device-resident where the host can write it ----
// HZ_REQSLOT_DEVICE: fine-grained device memory the CPU writes through the PCIe BAR (large-BAR
// systems): the request is in HBM before the replay starts. HZ_REQSLOT_PINNED: pinned host memory the
// kernels read over PCIe (zero-copy), the fallback when the device is not host-writable.
enum { HZ_REQSLOT_PINNED = 0, HZ_REQSLOT_DEVICE = 1 };
// 1: this device's memory is host-writable (large BAR, and the runtime reports a host address for a
// test allocation). Never dereferences anything; cached per device. HIPZAP_REQSLOT=host: always 0.
int hz_reqslot_probe(void);
// *dev = the address kernels read, *host = the address the CPU writes (write-only for a device slot:
// hz_reqslot_write), *kind = HZ_REQSLOT_*. A device slot when the probe says yes and the allocation's
// own host address is reported; else a pinned buffer (dev == host). Zero-filled. 0 or a HIP error.
int hz_reqslot_alloc(uint64_t bytes, void** dev, void** host, int* kind);
int hz_reqslot_free(void* dev, int kind);
// streaming, write-only copy of n bytes to a device slot's host address (csrc/reqcopy.h) + store
// fence; cap = bytes of the slot from dst on. The executor's copy for device-resident inputs.
void hz_reqslot_write(void* dst, const void* src, uint64_t n, uint64_t cap);
// host cost of one payload copy (us: out[0] best, out[1] median of `iters`), `threads` at once, each
// into its own slot[t]; streaming = hz_reqslot_write, else memcpy (profiles/reqslot)
int hz_reqslot_copy_bench(void** slots, const void* src, uint64_t n, int threads, int iters, int streaming,
                          double* out);
// diagnostics (csrc/diag.hip): kind 0 = no-op kernel, 1 = copy `bytes` from a to b
int hz_diag_launch(int kind, int blocks, int threads, void* a, void* b, long bytes, hipStream_t st);

// ---- plan images (csrc/plan.cpp, engine/plan.py): serialised bound programs ----
// bump HZ_ABI_EPOCH when a kernel's parameter SEMANTICS change without a size change
#define HZ_ABI_EPOCH 2
// op types of a plan image (1..5 were the per-op types of format version 1)
enum { HZ_PLAN_OP_MEMCPY = 6, HZ_PLAN_OP_KERNEL = 7, HZ_PLAN_OP_FORK = 8, HZ_PLAN_OP_JOIN = 9 };
typedef struct HzMemcpyArgs {
  void* dst;
  const void* src;
  uint64_t bytes;
} HzMemcpyArgs;
// load-phase timings (ms) reported by hz_plan_open / hz_plan_timings
enum { HZ_PLAN_T_PARSE = 0, HZ_PLAN_T_HIP_INIT = 1, HZ_PLAN_T_UPLOAD = 2, HZ_PLAN_T_CTX_ALLOC = 3,
       HZ_PLAN_T_BIND = 4, HZ_PLAN_T_CAPTURE = 5, HZ_PLAN_T_BLOB_ALLOC = 6,
       HZ_PLAN_T_FIRST_COPY = 7,
       // sub-phases of HZ_PLAN_T_UPLOAD (cold-start phase table): stream creation, the blob's
       // read + DMA, the wait for the device-code warm thread; and that thread's own duration
       HZ_PLAN_T_STREAM = 8, HZ_PLAN_T_UPLOAD_DMA = 9, HZ_PLAN_T_WARM_WAIT = 10, HZ_PLAN_T_WARM_THREAD = 11,
       HZ_PLAN_NT = 12 };
uint64_t hz_abi_version(void);
const char* hz_plan_last_error(void);
// read_blob = 0: allocate the weight blob but leave it unfilled (an RCCL broadcast fills it)
void* hz_plan_open(const char* path, int device, int read_blob, double* timings);
int hz_plan_add_contexts(void* plan, int n, int capture);
int hz_plan_num_contexts(void* plan);
// contexts added after this call (except one on the upload stream) get highest-priority streams
void hz_plan_set_stream_priority(void* plan, int high);
void hz_plan_timings(void* plan, double* out);
void* hz_plan_blob(void* plan, uint64_t* bytes);
void* hz_plan_host(void* plan, int ctx);
void* hz_plan_device(void* plan, int ctx);
void* hz_plan_stream(void* plan, int ctx);
void* hz_plan_upload_stream(void* plan);
int hz_plan_replay(void* plan, int ctx);
int hz_plan_sync(void* plan, int ctx);
int hz_plan_infer(void* plan, int ctx, const void* in, uint64_t in_off, uint64_t in_bytes, void* out,
                  uint64_t out_off, uint64_t out_bytes);
double hz_plan_bench(void* plan, int iters);
HzProgram hz_plan_prog(void* plan, int ctx);
int hz_plan_capture_ctx(void* plan, int ctx);

// ---- request executor (csrc/executor.cpp): one worker thread submits + polls completions ----
// host_in[k * n + i] = context i's pinned input k (n_in <= 4); host_out[i] = its pinned output
void* hz_exec_create(HzProgram* progs, hipStream_t* streams, void** host_in, const uint64_t* in_bytes, int n_in,
                     void** host_out, uint64_t out_bytes, int n);
// blocking: one request (in[k] = payload of input k), result copied to out; latency in *lat_us
void* hz_exec_create_batched(HzProgram* progs, hipStream_t* streams, void** host_in, const uint64_t* in_bytes,
                             int n_in, void** host_out, uint64_t out_bytes, int n, int rows, double max_wait_us,
                             int min_inflight);
// input k of every slot is a device-resident request slot (HZ_REQSLOT_DEVICE; host_in = its host
// address): payloads go in with the streaming write-only copy instead of memcpy. Before any submit.
int hz_exec_set_input_kind(void* exec, int k, int kind);
void hz_exec_batches(void* exec, uint64_t* batches);
int hz_exec_submit(void* exec, const void* const* in, void* out, double* lat_us);
int hz_exec_submit_rows(void* exec, const void* const* in, int m, void* out, double* lat_us);
// like hz_exec_submit (per-request executors only), copying nbytes[k] <= in_bytes[k] of input k: a
// request smaller than its pinned input (an image below the resize plan's maximum) pays for its own bytes
int hz_exec_submit_sized(void* exec, const void* const* in, const uint64_t* nbytes, void* out, double* lat_us);
void hz_exec_stats(void* exec, uint64_t* served, uint64_t* polls);
void hz_exec_destroy(void* exec);
int hz_exec_bench(void* exec, int clients, int iters, const void* const* in, double* lat_us, double* wall_us);

// ---- native HTTP/1.1 front end (csrc/http.cpp): POST /predict fast path + WSGI callback ----
typedef void (*HzHttpPyHandler)(void* req, const char* method, const char* target, const char* headers,
                                uint64_t hlen, const char* body, uint64_t blen);
void* hz_http_start(int listen_fd, HzHttpPyHandler py);
int hz_http_set_fast(void* srv, void* exec, int H, int W, int C, int out_floats, int classes, int probs,
                     const char* model);
// the native GET /inference route (csrc/http.cpp try_lm); sched = NULL removes it
int hz_http_set_lm(void* srv, void* sched, int V, int maxn, int dflt, int empty_id, const char* blob, uint64_t blen,
                   const uint8_t* flags);
void hz_http_respond(void* req, int status, const char* headers, uint64_t hlen, const char* body, uint64_t blen);
void hz_http_stats(void* srv, uint64_t* out4);
int hz_http_stop(void* srv);  // 1: all connections ended; 0: some still live (state leaked)
void hz_plan_close(void* plan);

#ifdef __cplusplus
}
#endif
