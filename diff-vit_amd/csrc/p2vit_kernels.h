// internal launch interface between the C ABI (p2vit_capi.cpp) and the kernels (p2vit_gemm.hip, p2vit_ln.hip, p2vit_attn.hip, p2vit_misc.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/p2vit.h"

#define GBK_PAD 64   // K granularity of the GEMM tiles: weights/activations are padded to this
#define P2V_EPI_F32 7     // internal: the layer output fmaf(acc, colscale, bias) as fp32, no QAct (taps of p2v_forward_linear_taps)

struct GemmArgs {
  const int8_t* A;      // activations [M][lda] int8
  int lda, M;
  const int8_t* W;      // weight codes [n_pad][K] int8, or (w4) packed int4 tiles [n_pad/128][K/64][128][32 B]
  int K, N;
  int w4;               // 1: W is the packed int4 layout (p2v_linear.packed4)
  const float* colscale;
  const float* bias;
  p2v_epilogue ep;
  void* out;
  int ldo;
  int8_t* out_codes;
  int8_t* out_codes2;   // EMBED tap only: the qact_embed codes (out_codes: the patch_embed.qact codes), both [rows of out][ldo]
  int tiles_n;          // filled by the launcher
#ifdef P2V_DIAG
  unsigned long long* stamps;   // diagnostic build only: per-workgroup cycle stamps (6 per workgroup) or null
#endif
};

// LayerNorm constants folded ahead of the launches (p2v_ln.pre, include/p2vit.h) instead of by every workgroup (ln_prepare).
// gm == nullptr: the kernel folds them itself.
typedef p2v_ln_pre LnPre;

struct LnArgs {
  const int8_t* x;
  long long row_stride;
  long long rows;
  int C;
  p2v_ln ln;
  int8_t* out;
  long long out_stride;
  int rows_per_half;    // filled by the launcher: consecutive rows per 32-lane half wave
  int force_generic;    // filled by the launcher (P2V_LN_GENERIC=1: A/B and parity runs of the generic chain)
  LnPre pre;            // optional, see above
  float* tap_out;       // optional: fp32 [rows][C], the unclamped integer output times out_scale (k_int_layernorm's TAP form, C <= 2048)
};

// AttnKArgs is the kernel argument of every UNTAPPED attention instantiation: its layout stays as it is, so that those kernels compile to
// the code they had; the tapped instantiations take AttnArgs, which the host side passes around (it converts to its base at the launch)
struct AttnKArgs {
  const int8_t* qkv;
  int B, N, H;
  p2v_attn at;
  int8_t* out;
  int8_t* probs_k;
  int pshift;           // filled by the launcher: score multiplier = 2^-pshift (>= 1) -> integer requant path; 0 = fp32 path
  int nq;               // query rows to compute, in whole 16-row blocks (0 = all): the resident and the packed kernel; the streaming kernel computes all rows
  int klim;             // 2^softmax_bits (8 or 16): the probability is 0 from k = klim on.  0 (an argument built without it) = 16: every launcher
                        // that takes AttnArgs from outside its file fills it in (p2v_attn_klim) and refuses any other value
#ifdef P2V_DIAG
  unsigned long long* stamps;   // diagnostic build only: 16 cycle stamps per workgroup (wave 0) or null
#endif
};
struct AttnArgs : AttnKArgs {
  // pitched taps (p2v_lis_attention_taps; each optional): [B][H][N][pitch] int8, pitch >= N a multiple of 16; only the columns [0, N) of a
  // row are written.  Any of them (or probs_k) selects the TAP instantiation
  int8_t* score_codes;  // qact_attn1 codes of every (query, key) pair
  int8_t* probs_kp;     // the exponents of probs_k in the pitched layout
  int pitch;
  bool tapped() const { return probs_k || score_codes || probs_kp; }
};

// klim as the kernels read it: 0 -> 16; -1 for anything but 8 and 16
inline int p2v_attn_klim(int klim) { return klim == 0 ? 16 : ((klim == 8 || klim == 16) ? klim : -1); }

struct WinAttnKArgs {      // the untapped instantiations' argument, as AttnKArgs
  const int8_t* qkv;
  int B, T, H;          // images, tokens per image, heads
  p2v_winattn wa;
  int8_t* out;
  int8_t* probs_k;
  int klim;             // 2^softmax_bits (8 or 16), as AttnKArgs.klim.  0 = 16: p2v_launch_window_attention (the one way in) fills it in
};
struct WinAttnArgs : WinAttnKArgs {
  // pitched taps (p2v_window_attention_taps; each optional): [B][n_windows][H][N][pitch] int8, pitch >= N a multiple of 16; only the
  // columns [0, N) of a row are written.  Any of them (or probs_k) selects the TAP instantiation
  int8_t* attn1_codes;  // qact_attn1 codes
  int8_t* qact2_codes;  // qact2 codes: behind the bias-table add, in front of the mask
  int8_t* probs_kp;     // the exponents of probs_k in the pitched layout
  int pitch;
  bool tapped() const { return probs_k || attn1_codes || qact2_codes || probs_kp; }
};
int p2v_launch_patch_merge_gather(const int8_t* x, int B, int H, int W, int C, int8_t* out, hipStream_t st);
int p2v_launch_avgpool_quant(const int8_t* x, int B, int T, int C, float s_in, float inv_s_out, int8_t* out, hipStream_t st);
int p2v_launch_window_attention(const WinAttnArgs& a, hipStream_t st);

int p2v_launch_patchify(const float* img, int B, int C, int H, int W, int P, float inv_s, int8_t* out, int k_pad, hipStream_t st);
int p2v_launch_fill_cls(int8_t* x, int B, int T, int D, const int8_t* cls, hipStream_t st);
// fp32 image x fake-quantised conv weights (input_quant = False): EMBED epilogue, g.A unused, g.W unpacked int8 codes [n_pad][K]
int p2v_launch_embed_fp32(const float* img, int B, int C, int H, int W, int P, const GemmArgs& g, hipStream_t st);
// uint8 input (p2v_forward_u8): the patch matrix through the int8 table [C][256] (-3: table + one patch exceed 64 KB of LDS), and the
// fp32-image convolution through the fp32 table [C][256]; nhwc: 1 = [B][H][W][C], 0 = [B][C][H][W]
int p2v_launch_u8_patchify(const uint8_t* img, int B, int C, int H, int W, int P, int nhwc, const int8_t* lut, int8_t* out, int k_pad,
                           hipStream_t st);
int p2v_launch_embed_u8(const uint8_t* img, int nhwc, const float* lut, int B, int C, int H, int W, int P, const GemmArgs& g, hipStream_t st);
int p2v_launch_gemm(int epi, const GemmArgs& g, hipStream_t st);     // -4: M * lda + K or the padded weight matrix reaches 2^32 bytes (tiled kernel)
// the few-rows kernel (p2vit_gemm_rows.hip): REQUANT / GELU / RESID at any M, parallel over N and K; -3: not one of its epilogues
int p2v_launch_gemm_rows(int epi, const GemmArgs& g, hipStream_t st);
// table of the pre-folded RESID epilogue (p2v_epilogue.resid_tab): [ceil(N/128)][6][128] floats; flags: dev [2] preset to {1, 0}
int p2v_launch_resid_prefold(const p2v_linear& lin, const p2v_epilogue& ep, int N, float* tab, unsigned* flags, hipStream_t st);
#define P2V_LN_MAX_C 4096   // channels of a LayerNorm row: k_int_layernorm up to 2048, k_int_layernorm_xwide beyond
int p2v_launch_layernorm(const LnArgs& a, hipStream_t st);
// rows of 2049 .. 4096 channels, a row per workgroup (p2vit_ln_xwide.hip); p2v_launch_layernorm routes to it with force_generic / pre filled
int p2v_launch_layernorm_xwide(const LnArgs& a, hipStream_t st);
bool p2v_ln_gemm_supported(int epi, int C, int N, int table_cells);
int p2v_launch_ln_gemm(int epi, const LnArgs& a, const GemmArgs& g, hipStream_t st);   // -3: shape not fused
int p2v_launch_attention(const AttnArgs& a, int head_dim, hipStream_t st);
int p2v_launch_attention_stream(const AttnArgs& a, int head_dim, hipStream_t st);   // any token count up to P2V_MAX_TOKENS_STREAMED (p2vit_attn_stream.hip)
int p2v_launch_attention_packed(const AttnArgs& a, hipStream_t st);   // head_dim 64, no tap, 609 .. P2V_MAX_TOKENS_PACKED tokens (p2vit_attn_packed.hip); the lower end is p2v_attention_kernel_of's: the launcher itself refuses only what has no instantiation (below 10 groups of 64 keys)
// which kernel p2v_launch_attention takes under the current switches: the P2V_KERNEL_* values of include/p2vit.h, -1 = refused (p2vit_attn.hip)
int p2v_attention_kernel_of(int head_dim, int tokens, int tapped);
// tokens per image the resident attention kernel covers (K / V^T of a head in LDS: 3 * head_dim bytes per key); 0: head_dim not instantiated
inline int p2v_resident_tokens_of(int head_dim) {
  if (head_dim == 32 || head_dim == 48 || head_dim == 64 || head_dim == 80) return P2V_MAX_TOKENS;
  return head_dim == 96 ? 17 * 32 : (head_dim == 128 ? 12 * 32 : 0);
}
int p2v_launch_stream_probe(int kernels, int usec, int workgroups, int lds_bytes, hipStream_t st);     // trains of one-wave timed waits (p2vit_misc.hip)
int p2v_launch_fake_quant(const float* x, long long n, const float* scale, int n_scale, long long inner, int lo, int hi,
                          float* out, int8_t* codes, hipStream_t st);
int p2v_launch_gelu_quant(const float* y, long long n, float inv_s, int8_t* codes, unsigned long long* flags, int force_slow,
                          hipStream_t st);
int p2v_launch_gelu_sweep(unsigned first_bits, unsigned count, float* max_err, hipStream_t st);
// exact GELU->requant threshold table (see the GELU section of p2vit_device.h)
int p2v_launch_gelu_table_build(float inv_s, const p2v_gelu_tab& t, unsigned* scratch, hipStream_t st);
int p2v_launch_gelu_table_check(float inv_s, const p2v_gelu_tab& t, unsigned long long* mismatches, hipStream_t st);

// CKA grams (p2vit_cka.hip): one record per layer in the workspace, and where the workspace's parts start
#include <vector>
struct CkaDesc {
  const float* x;
  const float* y;        // == x for X X^T
  long long F, ldx, ldy;
  long long item0;       // first workgroup of the layer in k_cka_partial's grid
  long long part0;       // first float of the layer's chunk partials
  int nchunks, sym, vec, pad;
};
struct CkaLayout {
  long long items;       // workgroups of k_cka_partial
  size_t desc_off, part_off, g64_off, total;
};
CkaLayout p2v_cka_layout(const p2v_cka_layer* layers, int L, int n, std::vector<CkaDesc>* descs);
int p2v_launch_cka_grams(const std::vector<CkaDesc>& descs, const CkaLayout& w, int n, float* grams, void* ws, hipStream_t st);
// the raw form p2v_code_grams takes for an fp32 stage: k_cka_partial and k_cka_reduce of ONE layer, the uncentred fp64 Gram (zero diagonal) to g64
int p2v_launch_cka_raw(const CkaDesc& desc, const CkaLayout& w, int n, double* g64, void* ws, hipStream_t st);
int p2v_launch_hsic(const float* g1, int l1, const float* g2, int l2, int n, void* acc, void* self1, void* self2, int dtype, hipStream_t st);

// pair-cosine sums of the DDV model diff (p2vit_ddv.hip): one record per stage
#define P2V_COS_I8_DEQ 64  // internal dtype of p2v_launch_pair_cosine_one: int8 codes, every value the fp32 product RN(code * scale[c]) (scale required)
struct CosDesc {
  const void* a;
  const void* b;
  const float* scale;    // per-channel fp32 [cols] (int8 only) or null
  long long sample_stride, row_stride;   // in elements
  long long item0;       // first workgroup of the stage in k_cos_partial's grid (0 for a stage launched alone)
  int rows, cols;
  int dtype;             // P2V_COS_I8 / P2V_COS_F32 / P2V_COS_LOG2K (p2v_launch_pair_cosine_one: also P2V_COS_I8_DEQ)
  int vec;               // pointers and strides are 16-byte aligned: whole column groups are read with one 16-byte load
  int nsplit;            // workgroups per sample
  int rows_per_split;
};
struct CosLayout {
  long long items;       // workgroups of k_cos_partial
  size_t desc_off, part_off, total;
};
CosDesc p2v_cos_desc(const p2v_cos_layer& a, int n, long long item0);
CosLayout p2v_cos_layout(const p2v_cos_layer* layers, int L, int n, std::vector<CosDesc>* descs);
int p2v_launch_pair_cosine(const std::vector<CosDesc>& descs, const CosLayout& w, int n, double* sums, void* ws, hipStream_t st);
int p2v_launch_pair_cosine_one(const CosDesc& d, int n, unsigned long long* partials, double* sums, hipStream_t st);
// recorded sequences (P2V_OP_COS / P2V_OP_COS_COMBINE): the records live in a device table built by p2v_cos_stage_descs
int p2v_launch_cos_stage(const CosDesc* desc_dev, long long items, unsigned long long* partials, hipStream_t st);
int p2v_launch_cos_combine(const CosDesc* descs_dev, int L, int n, const unsigned long long* partials, double* sums, hipStream_t st);

// stage statistics (p2vit_stats.hip): one plane into one record (p2v_code_stats / p2v_forward_stats / P2V_OP_STATS)
struct StatsDesc {
  const void* base;
  void* rec;             // the record (p2v_stats_bytes(cols)), accumulated into
  long long sample_stride, row_stride;   // in elements
  long long flat_rows;   // samples * rows (< 2^31): the plane as one list of rows
  int rows, cols;
  int kind;              // P2V_STAT_*
  int vec;               // base and strides are 16-byte aligned: whole column groups are read with one 16-byte load
  int tiles;             // column tiles of 1024
  int nsplit;            // row ranges; the grid is tiles * nsplit
  int rows_per_split;    // <= 2^16
};
StatsDesc p2v_stats_desc(const p2v_stat_layer& l, void* rec);
int p2v_launch_stats(const StatsDesc& d, hipStream_t st);
int p2v_launch_stats_init(void* rec, size_t bytes, int kind, int cols, hipStream_t st);

// integer Grams of a stage's codes (p2vit_gram.hip): one record per stage, passed to the launches by value
struct GramDesc {
  const int8_t* base;
  const uint8_t* shift;  // per-column exponents m_c [cols] or null
  long long sample_stride, row_stride;   // in elements
  long long groups;      // rows * cg: the 16-byte column groups of a sample (its features, rows padded to whole groups)
  int rows, cols;
  int cg;                // column groups per row
  int nchunks;           // chunks of P2V_GRAM_CHUNK / 16 groups
  int vec;               // base and strides are 16-byte aligned: whole column groups are read with one 16-byte load
};
GramDesc p2v_gram_desc(const p2v_gram_layer& l);
long long p2v_gram_items(const GramDesc& d, int n);    // workgroups of k_gram_partial = int64 [32][32] partial tiles
int p2v_launch_gram_i8(const GramDesc& d, int n, long long* partials, double* G, hipStream_t st);
int p2v_launch_gram_centre(const double* raw, long long pitch, long long layer_stride, int L, int n, float* grams, hipStream_t st);

// scoring of the logits (p2vit_score.hip): one record per row, then the fold into a totals slot (p2v_score_logits / p2v_score_accumulate)
int p2v_launch_score_rows(const float* logits, long long ld, int rows, int classes, const long long* labels, int* ranks, double* loss,
                          hipStream_t st);
int p2v_launch_score_accumulate(const int* ranks, const double* loss, int rows, const int* ks, int n_k, void* totals, hipStream_t st);

// search-based profiling inputs (p2vit_profile.hip): the state block of p2v_profile_* and its launches
struct ProfLayout {        // offsets into the state block; doubles first, then the fp32 tables
  int n, classes;
  long long d[2], g[2], rowd[2], rowg[2];      // in doubles: D [n][n], g [n], rowd [2][n], rowg [2] per model; the score is double 0
  long long o[2], o0[2];                        // in floats from the block's start: O [n][classes], O0 [n][classes] per model
  long long bytes;
};
ProfLayout p2v_profile_layout(int n, int classes);
int p2v_launch_profile_init(void* state, int n, int classes, const float* logits1, const float* logits2, hipStream_t st);
int p2v_launch_profile_candidates(const float* inputs, long long elems, int idx, long long pos, float eps, float* staging, hipStream_t st);
int p2v_launch_profile_step(void* state, int n, int classes, const float* cand1, const float* cand2, const float* staging, float* inputs,
                            long long elems, int idx, long long pos, double* trace, hipStream_t st);
int p2v_launch_profile_diversity(const float* logits, long long ld, int n, int classes, double* ws, double* out, hipStream_t st);

// weight freeze (p2vit_freeze.hip): one streaming launch, every argument checked by p2v_freeze_weights
int p2v_launch_freeze_weights(const float* w, long long ldw, int N, int K, const float* scale, int n_scale, int bits, int layout, void* out,
                              hipStream_t st);

// float LayerNorm -> QAct and table-softmax attention (p2vit_float_ln.hip, p2vit_attn_softmax.hip): the two operators of the
// Config(ptf=False) / Config(lis=False) plans
struct FloatLnArgs {
  const int8_t* x;
  long long row_stride;
  long long rows;
  int C;
  double s_in, eps;     // fp32 values of the caller, widened
  const float* gamma;
  const float* beta;
  const float* g;       // [C] output multiplier 1 / (channel_scale * s_out), a power of two
  int8_t* out;
  long long out_stride;
  float* tap_out;       // optional: fp32 [rows][C], RN of the fp64 LayerNorm value
};
struct SmAttnArgs {
  const int8_t* qkv;
  int B, N, H;
  float s_qkv_sq, qk_scale, inv_s_attn, av_mul;
  const unsigned* tab;  // dev [256]: fixed-point exp of max - code, entries below 2^21
  int8_t* out;
  int8_t* score_codes;  // optional pitched tap [B][H][N][pitch] of the qact_attn1 codes
  int pitch;
  int nq;               // query rows to compute in whole 16-row blocks (0 = all)
};
int p2v_launch_float_layernorm(const FloatLnArgs& a, hipStream_t st);          // picks the kernel by C; -1: C outside 4 .. 4096
int p2v_launch_float_layernorm_xwide(const FloatLnArgs& a, hipStream_t st);    // 2052 .. 4096 channels, a row per workgroup
// head_dim 32 / 64, 1 .. P2V_MAX_TOKENS tokens; -1: no instantiation
int p2v_launch_softmax_attention(const SmAttnArgs& a, int head_dim, hipStream_t st);
// Swin window attention with the table softmax (p2vit_winattn_softmax.hip): Config(lis=False) of a Swin plan
struct WinSmArgs {
  const int8_t* qkv;
  int B, T, H;          // images, tokens per image, heads
  p2v_winattn wa;       // x0_int / b_int / c_int are not read
  const unsigned* tab;  // dev [256]: fixed-point exp of (max - code) * s_q2, entries below 2^21
  int8_t* out;
};
// head_dim 32, windows of 1 x 1 ... 12 x 12; -1: no instantiation
int p2v_launch_window_softmax_attention(const WinSmArgs& a, hipStream_t st);

// patch-similarity entropy and its gradient (p2vit_psaq.hip): the workspace sections in bytes from its 256-byte aligned start
#define PSAQ_POINTS 10      // points of the density (generate_data.py:110)
#define PSAQ_CHUNK 4096     // similarities per fp64 partial of the point sums
struct PsaqLayout {
  long long sims, ahat, norms, mm, range, psums, coef;   // S [B*G][T][T], A^ [B*G][T][hd], |a| [B*G][T], min / max partials, lo / hi, point-sum partials, coefficients
  int sim_blocks, chunks;                                // workgroups of S per group, chunks per image
  long long bytes;
};
struct PsaqArgs {
  const float* av;
  int B, G, H, N, hd;
};
PsaqLayout p2v_psaq_layout(int B, int G, int N, int hd);
// -1: a launch grid beyond 2^31 workgroups
int p2v_launch_psaq(const PsaqArgs& a, void* ws, double* value, float* grad, hipStream_t st);

// Hutchinson bookkeeping (p2vit_hessian.hip): segments per launch - their table is the launch's kernel argument
#define HS_MAX_SEGS 64
size_t p2v_hs_state_bytes(int n_layers);
long long p2v_hs_dot_chunks(const p2v_seg2* segs, int n_segs);          // fp64 partials p2v_launch_group_dot writes
int p2v_launch_rademacher_fill(const p2v_seg* segs, int n_segs, unsigned long long seed, unsigned long long probe, hipStream_t st);
// state == nullptr: the sums alone; else the stopping update of layer s with (probe, tol) behind out[s]
int p2v_launch_group_dot(const p2v_seg2* segs, int n_segs, double* out, double* partials, void* state, int probe, double tol, hipStream_t st);
int p2v_launch_hutchinson_init(void* state, int n_layers, hipStream_t st);
