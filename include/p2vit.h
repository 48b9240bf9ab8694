/*
 * p2vit.h -- C ABI of the MI355X-native PoT-PTQ quantized ViT forward engine (libp2vit_hip.so).
 *
 * Drop-in boundary.  The reference (LeSN-Lab/diff-ViT) has no native code: its boundary is the Python
 * nn.Module surface of models/ptq/layers.py plus VisionTransformer.forward (models/vit_fquant.py:780).
 * This header is what a ctypes/cffi binding inside that surface calls when `.quant` is on; every entry
 * point names the reference function(s) it replaces.  Signatures carry only PODs, device pointers and a
 * hipStream_t (passed as void*): no torch types.
 *
 * Conventions
 *   - every pointer marked "dev" is a device (HBM) pointer borrowed for the duration of the call (plan
 *     setters: for the lifetime of the plan); the library never allocates or frees device memory and
 *     never synchronises; work is enqueued on `stream`.
 *   - return value: 0 = ok, negative = error (P2V_E_*); p2v_last_error() gives the message of the last
 *     failing call on the calling thread.  The Python shim maps P2V_E_BITS -> ValueError/KeyError (as
 *     bit_pool.index / BIT_TYPE_DICT lookups do, vit_fquant.py:282, layers.py:174), P2V_E_SHAPE ->
 *     AssertionError (layers_quant.py:437), P2V_E_UNSUPPORTED -> NotImplementedError (quantizer/base.py:28).
 *   - HIP graph capture (hipStreamBeginCapture on `stream`, torch.cuda.graph): an entry point that only launches kernels and
 *     hipMemsetAsync on `stream`, with every argument passed by value or pointing at memory that outlives the call, can be recorded and
 *     replayed: the whole-model forwards (p2v_forward, _u8, _taps, _linear_taps, p2v_forward_ddv / _ex / _ex2, p2v_forward_stats; p2v_forward_many / _many_u8, whose
 *     device-to-device copies on `stream` are recorded with the launches), p2v_run_ops
 *     and every per-operator entry point not named below.  HOST arguments (bit_config, the p2v_op table, tap pointer arrays, p2v_* structs)
 *     are read when the call is made, i.e. baked into the graph.  The entry points that copy from host memory of their own, read results
 *     back, allocate, or time with events cannot be recorded - a capture records work, it does not run it - and return
 *     P2V_E_UNSUPPORTED ("... the stream is capturing a HIP graph ...") while `stream` is capturing, after their argument checks, with
 *     nothing enqueued and the capture left valid: p2v_pair_cosine, p2v_cka_grams, p2v_code_grams, p2v_forward_grams, p2v_forward_profile,
 *     p2v_forward_profile_begin / _end (the token stays valid), p2v_run_ops_profile, p2v_gelu_table_build, p2v_resid_prefold.  A capture
 *     status that cannot be read is not taken as capturing.  The plan-time calls that take no stream and synchronise the device
 *     (p2v_plan_set_block, p2v_plan_set_linear, p2v_plan_set_head, p2v_plan_set_float_block, p2v_ln_prefold, p2v_plan_prepare_grams) and
 *     p2v_plan_create / _destroy belong in front of any capture; they have no stream to ask.  A new refusal is no ABI change.
 *     (tests/test_graph_capture_gpu.py; the table of every entry point is in DESIGN.md, "Graph capture of the forwards".)
 *   - activations between kernels are int8 codes, row-major [rows][channels]; "rows" = batch*tokens.
 *   - all scales named *_pot are exact powers of two (the reference's PoT observers, minmax.py:247-251);
 *     per-channel PTF scales (ptf.py:51,133) are arbitrary fp32 and are divided by, as the reference does.
 *   - output footprint: an entry point writes the elements of its result and nothing else - no byte in front of the first or behind the
 *     last row, and where rows are strided (ldo, out_stride, p2v_winattn.out_stride) no byte of the padding between them, which keeps what
 *     the caller put there.  Particulars, stated at the entry points: the patchify entry points write zeros to the columns [C*P*P, k_pad);
 *     P2V_EPI_EMBED leaves the class-token rows alone; optional side outputs (tap_out, out_codes, ln_out, probs_k) are dense results with
 *     the same rule.  Input padding - the bytes between rows when lda / row_stride / qkv_stride exceed the row, and the columns [width, K) a
 *     contraction walks through zero weight columns - may hold anything: it never reaches a result.
 *     (tests/test_kernel_edges_gpu.py runs the per-operator entry points listed below into sentinel-filled buffers, and the class-token
 *     fill of p2v_forward on a sentinel-filled workspace.)
 *     The whole-model entry points (p2v_forward, p2v_forward_u8, p2v_forward_taps, p2v_forward_linear_taps, p2v_forward_ddv / _ex) compose
 *     these launches inside the caller's workspace, and two statements hold for them:
 *       (1) a forward's result - logits, taps, sums - does not depend on what the workspace holds on entry: it may be uninitialised, or
 *           left over from another batch size, bit list or entry point.  Every byte a launch reads was written by an earlier launch of the
 *           same call or meets a zero weight column (the k-tile tail of a width that is no multiple of 64; the rows the class-row branch
 *           of the last block leaves stale are not read);
 *       (2) a forward writes nothing outside [workspace, workspace + p2v_workspace_bytes) - p2v_ddv_workspace_bytes for p2v_forward_ddv / _ex -
 *           and outside its dense outputs (logits [batch][classes], each tap at its stated extent, sums, tap_scratch up to
 *           p2v_ddv_tap_scratch_bytes, attn_scratch of p2v_forward_ddv_ex2 up to p2v_ddv_attn_scratch_bytes - and of its rows only the
 *           columns [0, tokens)).  Inside the workspace the alignment gaps between the seven buffers and the trailing 256 bytes are
 *           never written.  Each launch of a stop_after >= 0 run, where the last block computes every row, writes exactly the
 *           rows x cols extent of its target buffer(s) (p2v_workspace_view).  The class-row launches of a stop_after = -1 run write less
 *           ("cls_rows": `batch` compact rows of ln / hid, the class rows of x / att); for them the statement is the weaker one that
 *           they stay out of the gaps and the tail and change nothing outside the patch rows of x / att and the hid / ln buffers,
 *           against a cls_rows = 0 run.
 *     (tests/test_forward_state_gpu.py: workspace, logits, taps, sums and tap scratch in sentinel arenas under three fills, the write
 *     map launch by launch, one workspace through a history of calls, 2 / 5 / 10 tokens per image against the oracle.)
 *
 * Limits of what is instantiated (everything else returns P2V_E_UNSUPPORTED, at plan creation where the geometry is known):
 *   - ViT attention: head_dim 32, 48, 64, 80, 96 or 128 (round 4; before: 32 / 64); up to P2V_MAX_TOKENS_STREAMED = 4096 tokens per image.  Three
 *     kernels, chosen per launch (p2v_attention_kernel tells which), all with the same codes:
 *       resident - K / V^T (bf16) of an image's head in LDS, a query block's scores in registers: up to P2V_MAX_TOKENS = 608 tokens (224^2 / 16 =
 *         197, 384^2 / 16 = 577, ...), 544 at head_dim 96, 384 at head_dim 128 (p2v_resident_tokens);
 *       packed - head_dim 64 without the probs_k tap, beyond the resident kernel up to P2V_MAX_TOKENS_PACKED = 1216 tokens (448^2 / 16 = 785,
 *         512^2 / 16 = 1025; p2v_packed_tokens): K and V^T (int8) in LDS, score codes four to a register, P.V on the int8 MFMA;
 *       streaming - everything else up to 4096 tokens (other head dimensions beyond their resident limit, 1217 tokens and more, every launch
 *         with probs_k beyond the resident limit): re-reads K / V per query block (round 4: slow, exact, so that no geometry of the
 *         reference's VisionTransformer is refused);
 *     Swin window attention: head_dim 32, windows up to 12 x 12 (up to 8 x 8: one lane per token; 9 x 9 ... 12 x 12, the
 *     patch 4 / window 12 / 384^2 geometry: the kernel of csrc/p2vit_winattn_wide.hip, same codes);
 *   - embed_dim and MLP width of a plan: multiples of 16 (round 4; before: 64) - the contractions walk 64-deep k-tiles through zero weight
 *     columns (p2v_linear: k_pad = round_up(K, 64)); the per-operator GEMM entry points take K in whole k-tiles;
 *   - LayerNorm: up to 4096 channels as an operator (p2v_int_layernorm, P2V_OP_LAYERNORM, p2v_ln_prefold: up to 2048 a row per wave or
 *     half wave, beyond that a row per workgroup, csrc/p2vit_ln_xwide.hip - the 4 * 768 = 3072-channel PatchMerging norm of Swin-L); a
 *     p2v_plan (ViT) keeps embed_dim <= 2048.  PTF input masks (in_scale / min in_scale) in {1, 2, 4, 8}, and the row's sum of squares
 *     must fit 32 unsigned bits: C * (128 * largest mask)^2 < 2^32 (any mask up to C = 4092, masks <= 4 at C = 4096) - the caller's to
 *     check, the kernels do not;
 *   - LayerNorm output scale: p2v_ln.inv_out is MULTIPLIED by where the reference divides by the scale - identical for the power-of-two
 *     scales of this path; for any other scale pass p2v_ln.out_scale too and the kernel divides (exact, ABI 3);
 *   - REQUANT epilogues fold 1/scale into the column constants: it must be a power of two;
 *   - log-int-softmax constants: c_int < 2^24 (qact_attn1 scale >= 2^-11);
 *   - Config(ptf=False) / Config(lis=False) of a ViT / DeiT plan (p2v_plan_set_float_ops, at the end of this header): the table-softmax
 *     attention for head_dim 32 / 64 and up to P2V_MAX_TOKENS tokens; a p2v_plan (ViT) keeps embed_dim <= 2048;
 *   - float LayerNorm (p2v_float_layernorm, P2V_OP_FLOAT_LAYERNORM): 16 .. P2V_FLOAT_LN_MAX_C = 4096 channels, a multiple of 4, under one
 *     power-of-two input scale: up to 2048 a row per wave, 2052 .. 4096 a row per workgroup (csrc/p2vit_float_ln_xwide.hip - the 4 * 768 =
 *     3072-channel PatchMerging norm of Swin-L), whole rows only there (row_stride >= C);
 *   - Swin plans (recorded p2v_op sequences): lis = False through p2v_window_softmax_attention (head_dim 32, windows up to 12 x 12, qact2
 *     scale <= 2^-2); ptf = False through P2V_OP_FLOAT_LAYERNORM records at every LayerNorm, every other record unchanged (each PTF
 *     vector repeats one scale).
 */
#ifndef P2VIT_H
#define P2VIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P2V_ABI_VERSION 6
#define P2V_MAX_TOKENS 608            /* tokens per image of the RESIDENT ViT attention kernel (K / V^T of a head in LDS; 19 pairs of 32 keys) */
#define P2V_MAX_TOKENS_STREAMED 4096  /* tokens per image of the streaming attention kernel that takes over beyond the resident one's limit (round 4) */
#define P2V_MAX_TOKENS_PACKED 1216    /* tokens per image of the packed attention kernel (head_dim 64: K / V^T as int8 in LDS; 19 groups of 64 keys) */
/* tokens per image a plan / p2v_lis_attention accepts at this head dimension (P2V_MAX_TOKENS_STREAMED; 0: head_dim not instantiated), and how many of
 * them the resident (fast) kernel covers: 608 up to head_dim 80, 544 at 96, 384 at 128 - launches beyond run the packed or the streaming kernel */
int p2v_max_tokens(int head_dim);
int p2v_resident_tokens(int head_dim);
/* (additive) tokens per image the packed kernel covers beyond the resident one: P2V_MAX_TOKENS_PACKED at head_dim 64, 0 at every other */
int p2v_packed_tokens(int head_dim);
/* (additive) the kernel a p2v_lis_attention / p2v_lis_attention_rows / plan launch of this shape takes under the current switches
 * ("attn_stream", "attn_packed"); tapped: probs_k != NULL.  -1: the shape is refused (head_dim not instantiated, tokens outside 1 .. 4096).
 * It is the function the launcher itself asks. */
#define P2V_KERNEL_RESIDENT 0
#define P2V_KERNEL_PACKED 1
#define P2V_KERNEL_STREAMING 2
int p2v_attention_kernel(int head_dim, int tokens, int tapped);

enum {
  P2V_OK = 0,
  P2V_E_ARG = -1,         /* null pointer / bad size                                  */
  P2V_E_BITS = -2,        /* bit_config entry not in {4,8} or wrong length             */
  P2V_E_SHAPE = -3,       /* image / tensor shape does not match the plan              */
  P2V_E_UNSUPPORTED = -4, /* configuration the kernels are not instantiated for        */
  P2V_E_WORKSPACE = -5,   /* workspace too small                                       */
  P2V_E_LAUNCH = -6,      /* hipLaunch failure (message carries hipGetErrorString)     */
  P2V_E_STATE = -7        /* plan incomplete (a setter was not called)                 */
};

/* GEMM epilogues: what follows F.linear / F.conv2d in the reference graph. */
enum {
  P2V_EPI_REQUANT = 0, /* QLinear -> QAct (PoT): attn.qkv->qact1 (vit_fquant.py:293,307)                      */
  P2V_EPI_GELU = 1,    /* QLinear -> nn.GELU -> QAct (PoT): mlp.fc1->act->qact1 (layers_quant.py:316,331-333) */
  P2V_EPI_RESID = 2,   /* QLinear -> QAct(PTF) -> + residual -> QAct(PTF): proj->qact3->+x->Block.qact2
                          (vit_fquant.py:334-338,431) and fc2->qact2->+x->Block.qact4 (layers_quant.py:342-346,
                          vit_fquant.py:468)                                                                   */
  P2V_EPI_EMBED = 3,   /* QConv2d -> PatchEmbed.qact -> qact_embed -> + qact_pos(pos) -> qact1(PTF)
                          (layers_quant.py:467-491, vit_fquant.py:715-733)                                     */
  P2V_EPI_HEAD = 4     /* head -> act_out, fp32 logits on the int8 grid (vit_fquant.py:792-796)                */
};

typedef struct p2v_model_desc {
  int32_t abi_version; /* P2V_ABI_VERSION */
  int32_t img_size, patch_size, in_chans;
  int32_t embed_dim, depth, num_heads, mlp_hidden, num_classes;
} p2v_model_desc;

/* One fake-quantised weight matrix for one bit width (QLinear/QConv2d.forward, layers.py:82-88,173-178;
 * UniformQuantizer.quant, uniform.py:50-88).  packed4 == 0: codes one per byte ([-8,7] for 4-bit), row
 * major [n_pad][k_pad], n_pad = round_up(N,128), k_pad = round_up(K,64), zero padded.
 * packed4 == 1 (4-bit codes only): two codes per byte, stored as the LDS images of the GEMM's weight tiles --
 *   [n_pad/128 column tiles][k_pad/64 k-tiles][128 rows][32 bytes]; the 32 bytes of row r hold its 64 k-values as four 8-byte chunks
 *   c (k = 16c .. 16c+15) at chunk position c ^ ((r >> 3) & 3) (bank swizzle); inside a chunk byte j of dword 0 is
 *   code[j] | code[4+j] << 4 and byte j of dword 1 is code[8+j] | code[12+j] << 4 (low nibble first, two's complement nibbles).
 *   Half the bytes, one contiguous 4 KB block per tile; gfx950 has no int4 MFMA, the kernels widen the nibbles to int8 in registers.
 * colscale[n] = s_x * s_w[n]  (activation scale times per-tensor (int8) or per-out-channel (int4) weight
 * scale; both powers of two, so the product is exact).  bias is the un-quantised fp32 bias. */
typedef struct p2v_linear {
  const int8_t* w_codes; /* dev */
  const float* colscale; /* dev [n_pad] */
  const float* bias;     /* dev [n_pad] */
  const int8_t* w_frag;  /* dev, optional (NULL): the same codes in MFMA-fragment order for p2v_ln_gemm_i8 --
                          * [n_pad/128 column tiles][4 waves][k_pad/32 k-steps][64 lanes][16 bytes], lane = 32*h + r holding
                          * W[128*tile + 32*wave + r][32*kstep + 16*h .. +16): the A operand of v_mfma_i32_32x32x32_i8 as one
                          * coalesced 1 KB load per wave.  packed4 == 0: one code per byte (16 bytes per lane).  packed4 == 1 (ABI 4):
                          * the lane's 16 codes in 8 bytes, byte j of dword 0 = code[j] | code[4+j] << 4, of dword 1 =
                          * code[8+j] | code[12+j] << 4 (the chunk format of the packed tiles): half the weight bytes */
  int32_t packed4;       /* 1: w_codes is the packed int4 tile layout described above */
} p2v_linear;

/* QIntLayerNorm.forward mode 'int' (layers.py:255-289) fused with the division by the SmoothQuant
 * channel scale and the QAct that follows it (vit_fquant.py:284-289, layers_quant.py:305-311).
 *   x_q = code * mask[c];  mask[c] = round(in_scale[c] / s1), s1 = min_c in_scale[c]
 *   out = clamp(rne(LN_int(x_q) * post_mul[c]), -128, 127)
 * inv_out[c] = 1 / (out_quantizer.scale * out_quantizer_scale[c])  (a power of two in P2-ViT: multiplying by it IS the reference's
 *              division by the scale)
 * out_scale[c] = the scale itself, optional (NULL): needed only when it is NOT a power of two - the kernel then divides by it
 *              (IEEE) exactly where the reference does (layers.py:279-286); with NULL it multiplies by inv_out, which for such a
 *              scale lands the 8-bit multiplier M one step away on about 1e-5 of the elements
 * post_mul[c] = out_scale[c] / next_channel_scale[c] / next_act_scale  (power of two). */
/* Constants of a LayerNorm folded ahead of its launches (round 4, ABI 5; optional: gm == NULL and every kernel folds per workgroup, with the
 * same codes): gamma * inv_out and beta * inv_out, each padded with zeros to round_up(C, 256) channels, their extreme magnitudes and the two
 * tests of the fast chain (1 / out_scale a power of two everywhere; post_mul == 1 everywhere).  Filled by p2v_ln_prefold; the frozen plan of
 * p2v_forward folds its own copies and ignores what the caller passes here. */
typedef struct p2v_ln_pre {
  const float* gm;        /* dev [round_up(C, 256)] */
  const float* bt;        /* dev [round_up(C, 256)] */
  float gmin, gmax, bmax;
  int32_t pot, pm_one;
} p2v_ln_pre;

typedef struct p2v_ln {
  float s1;
  const float* mask;      /* dev [C] */
  const float* gamma;     /* dev [C] */
  const float* beta;      /* dev [C] */
  const float* inv_out;   /* dev [C] */
  const float* post_mul;  /* dev [C] */
  const float* out_scale; /* dev [C] or NULL (ABI 3) */
  p2v_ln_pre pre;         /* optional (ABI 5), see above */
} p2v_ln;
/* Fold the constants of *ln for C channels into buf (dev, p2v_ln_prefold_bytes(C) bytes, owned by the caller, must outlive the launches) and
 * set ln->pre.  Reads the arrays back to the host: synchronises the device; call it after the arrays have been written.  C: a positive
 * multiple of 4 up to 4096 (P2V_E_SHAPE otherwise). */
size_t p2v_ln_prefold_bytes(int C);
int p2v_ln_prefold(p2v_ln* ln, int C, float* buf, size_t buf_bytes);

/* (q @ k^T) * scale -> qact_attn1 -> QIntSoftmax (log-int-softmax, uint4) -> @ v -> qact2
 * (vit_fquant.py:309-326, layers.py:323-376). */
typedef struct p2v_attn {
  float s_qkv_sq;   /* s_q1^2                                      */
  float qk_scale;   /* head_dim^-0.5 (vit_fquant.py:74)            */
  float inv_s_attn; /* 1 / qact_attn1 scale (pot)                  */
  float av_mul;     /* s_q1 / qact2 scale (pot)                    */
  int32_t x0_int, b_int, c_int; /* I-BERT exp polynomial constants (layers.py:334-351) for sf = qact_attn1 scale */
} p2v_attn;

/* nn.GELU -> QAct(PoT) (layers_quant.py:331-333) as an exact threshold table built by p2v_gelu_table_build:
 *   u = y * k (exact: k is a power of two) of the fp32 pre-activation y;  cell i = clamp(floor(u) + off, 0, cells-1);
 *   entry = { float thr * k; uint32 lo | hi << 8 };  code = (u >= thr * k) ? (int8)hi : (int8)lo.
 *   (Round 4: the epilogues form u straight from the accumulator, fma(acc, colscale * k, bias * k) = RN(acc * colscale + bias) * k, and never
 *   y itself; before, the cell was floor(fma(y, k, off)) and the entry held thr.  A table must come from THIS library's builder.)
 *   table == NULL selects the arithmetic evaluation (A&S erfc + fp64 fallback). */
typedef struct p2v_gelu_tab {
  const void* table; /* dev [cells] 8-byte entries, or NULL */
  float k, off;      /* k = 2 / s_out (a power of two: y*k is exact), off = -floor(y_lo * k), an integer      */
  int32_t cells;
} p2v_gelu_tab;

/* Epilogue parameters; which members are read depends on the epilogue kind. */
typedef struct p2v_epilogue {
  float inv_s_out;       /* REQUANT/GELU/HEAD: 1/scale of the following QAct (pot)           */
  float s_out;           /* HEAD: act_out scale                                               */
  const float* s_mid;    /* dev [N] RESID: PTF scale of qact3 / mlp.qact2                    */
  const float* s_res;    /* dev [N] RESID: scale of the residual-stream codes being added     */
  const float* s_next;   /* dev [N] RESID/EMBED: PTF scale of the QAct that ends the stage    */
  const int8_t* residual;/* dev [M][N] RESID: residual-stream codes (may alias the output)    */
  /* EMBED only */
  float inv_s_pe;        /* 1 / PatchEmbed.qact scale                                         */
  float pe_to_embed;     /* PatchEmbed.qact scale / qact_embed scale                          */
  float s_embed;         /* qact_embed scale                                                  */
  const float* pos_deq;  /* dev [tokens][N]  qact_pos(pos_embed), dequantised                 */
  int32_t patches;       /* patches per image; output row = b*(patches+1) + 1 + p             */
  p2v_gelu_tab gelu;     /* GELU only: threshold table for inv_s_out (optional)              */
  float* tap_out;        /* REQUANT/GELU, optional: dev fp32 [M][N] receives the layer output BEFORE the
                            following QAct / GELU, acc*colscale + bias -- what the reference keeps as
                            Attention.qkv_output (vit_fquant.py:301) / Mlp.fc1_output (layers_quant.py:326) */
  const float* resid_tab;/* RESID, optional (ABI 5): dev table written by p2v_resid_prefold for THIS (weights, epilogue) pair, or NULL.
                            With it the launch runs the pre-folded epilogue (same codes, ~4 VALU instructions per output less); the
                            frozen plan of p2v_forward builds and owns its tables itself */
} p2v_epilogue;

/* RESID epilogue constants folded ahead of the launches (round 4).  The reference computes, per output channel n (vit_fquant.py:334-338,431;
 * layers_quant.py:342-346, vit_fquant.py:468),
 *     q3 = clamp(round((acc * colscale[n] + bias[n]) / s_mid[n]));   q = clamp(round((res * s_res[n] + q3 * s_mid[n]) / s_next[n]))
 * with two IEEE divisions by non-power-of-two PTF scales.  The table holds, per column tile of 128 channels, six arrays of 128 floats:
 *     colscale * fl(1/s_mid), bias * fl(1/s_mid), s_mid, s_res, rh = fl(1/s_next), rl = fl(1/s_next - rh)
 * (i)  the first quotient becomes ONE fma on the accumulator with the existing margin test (|t - rint t| < 0.5 - 1e-4, else the exact
 *      division): valid when colscale is a power of two and |bias / s_mid| <= 512, which bounds the error of the folded form by 7e-5;
 * (ii) the second quotient becomes xs * rh + xs * rl (a 48-bit reciprocal) WITHOUT a test: its numerator takes at most 65 536 values per
 *      channel (256 residual codes x 256 q3 codes), and p2v_resid_prefold evaluates every one of them on the device against the IEEE
 *      division - the table is usable only if all N x 65 536 results agree.
 * *usable = 0 (table not to be used; the generic RESID epilogue gives the same codes) when (i) or (ii) does not hold.
 * Synchronises `stream`.  tab: dev, p2v_resid_prefold_bytes(N) bytes, owned by the caller, must outlive the launches that use it. */
size_t p2v_resid_prefold_bytes(int N);
int p2v_resid_prefold(const p2v_linear* lin, const p2v_epilogue* epi, int N, float* tab, size_t tab_bytes, int* usable, void* stream);

typedef struct p2v_plan p2v_plan;

/* ---- whole-model entry points: VisionTransformer.forward in quant state (vit_fquant.py:700-799) ---- */
int p2v_plan_create(const p2v_model_desc* desc, p2v_plan** out);
void p2v_plan_destroy(p2v_plan* plan);

/* layer index follows the reference's bit_config order (vit_fquant.py:710-711,748,789):
 * 0 = patch embed, 1+4*i+{0,1,2,3} = block i {qkv, proj, fc1, fc2}, 4*depth+1 = head.  bits in {4,8}. */
int p2v_plan_set_linear(p2v_plan* plan, int layer, int bits, const p2v_linear* lin);

/* inv_s_input = 1 / qact_input scale; inv_s_input == 0 selects VisionTransformer(input_quant=False) (the reference's vit_large
 * factory, vit_fquant.py:925): no input QAct, the fp32 image feeds the fake-quantised convolution directly - fp64 accumulation of the
 * exact products, one rounding to fp32; the layer-0 weights must then be unpacked codes (packed4 = 0) with colscale = s_w.
 * embed epilogue constants (one set per patch-embed bit width index 0:4-bit 1:8-bit is not
 * needed: activation scales do not depend on the weight bits); cls row codes [D] after qact1. */
int p2v_plan_set_embed(p2v_plan* plan, float inv_s_input, const p2v_epilogue* embed_epi,
                       const int8_t* cls_row_codes /* dev [D] */);
/* Optional, additive (found by its symbol): the codes of the class row under qact_embed, clamp(round(cls_token / s_embed)), dev int8 [D] -
 * the constant row 0 of the `qact_embed` stage of P2V_DDV_STAGES_FULL (p2v_forward_ddv_ex fills it into the stage's plane with the
 * class-token fill kernel).  The array must outlive the plan.  Nothing else reads it. */
int p2v_plan_set_embed_tap_cls(p2v_plan* plan, const int8_t* cls_embed_codes /* dev [D] */);

/* per block, per bit-pool index (0: 4-bit, 1: 8-bit) of qkv (for ln1/attn side) and of fc1 (for ln2 side):
 * the reference keeps best_scale/best_act_scale per bit (vit_fquant.py:282-292, layers_quant.py:305-313). */
typedef struct p2v_block {
  p2v_ln ln1[2];            /* indexed by bit-pool index of qkv */
  float inv_s_qkv[2];       /* 1/attn.qact1 scale (same for both, kept per index for symmetry) */
  p2v_attn attn;
  p2v_epilogue proj_epi;    /* RESID */
  p2v_ln ln2[2][2];         /* [bit index of qkv (attn.channel_scale quirk, vit_fquant.py:464)][bit index of fc1] */
  float inv_s_fc1;          /* 1/mlp.qact1 scale */
  p2v_gelu_tab gelu_fc1;    /* threshold table of fc1 -> GELU -> qact1 for inv_s_fc1 (table may be NULL) */
  p2v_epilogue fc2_epi;     /* RESID */
} p2v_block;
/* Stores the block's constants (the arrays stay the caller's and must outlive the plan) and - since round 3 - reads the LayerNorm arrays
 * back once to fold gamma / out_scale and beta / out_scale and to run the fast-chain tests on the host, so that the kernels of p2v_forward
 * do not repeat that per workgroup.  The call therefore synchronises the device (hipDeviceSynchronize) and must come after the arrays have
 * been written; changing an array afterwards requires setting the block again.  The folded copies are owned by the plan and live on the
 * device that owns blk->ln1[0].gamma (found with hipPointerGetAttributes - the process's current device does not matter; all blocks of a
 * plan must live on one device).  If the fold cannot be done (a HIP error, arrays on another device than earlier blocks) the call still
 * returns P2V_OK - the kernels then fold per workgroup, with identical results - and leaves the reason in p2v_last_error();
 * p2v_plan_block_prefolded() tells which of the two a block got. */
int p2v_plan_set_block(p2v_plan* plan, int block, const p2v_block* blk);
/* (Round 4: p2v_plan_set_block and p2v_plan_set_linear also build the plan's RESID tables - p2v_resid_prefold for proj / fc2 of a block once
 * both the block and the layer's weights are set; a later change of either rebuilds them.  blk->proj_epi.resid_tab / fc2_epi.resid_tab are
 * ignored.) */
/* 1: the LayerNorm constants of the block were folded when it was set; 0: its kernels fold per workgroup (p2v_last_error() of the
 * p2v_plan_set_block call says why); negative: error. */
int p2v_plan_block_prefolded(const p2v_plan* plan, int block);
/* which RESID tables of the block are in use: bit 0 proj / 4-bit weights, bit 1 proj / 8-bit, bit 2 fc2 / 4-bit, bit 3 fc2 / 8-bit
 * (a clear bit of a layer whose weights are set: p2v_resid_prefold found the pre-folded form not provable, the generic epilogue runs). */
int p2v_plan_resid_prefolded(const p2v_plan* plan, int block);

int p2v_plan_set_head(p2v_plan* plan, const p2v_ln* final_ln, float inv_s_out, float s_out);

size_t p2v_workspace_bytes(const p2v_plan* plan, int batch);

/* images: dev fp32 [batch][in_chans][img][img];  bit_config: HOST int8 [n_cfg], n_cfg = 4*depth+2;
 * logits: dev fp32 [batch][num_classes].  stop_after < 0 runs everything; otherwise execution stops after
 * that many kernel launches (parity tests read the workspace buffers, see p2v_workspace_view).
 * With stop_after < 0 the last block runs behind its qkv GEMM on the class-token rows only (the logits read nothing else): the views
 * "x", "att", "hid" and "ln" then hold that block's values only where the logits need them; stop_after >= 0 is the way to read full
 * buffers (switch "cls_rows" of p2v_set_tuning). */
int p2v_forward(p2v_plan* plan, const float* images, int batch, const int8_t* bit_config, int n_cfg,
                float* logits, void* workspace, size_t workspace_bytes, int stop_after, void* stream);

/* p2v_forward with the activation taps of the analysis scripts (cka_utility.py:26-113 reads blocks[i].attn.qkv_output and
 * blocks[i].mlp.fc1_output): qkv_out / fc1_out are HOST arrays of `depth` device pointers (entries or the arrays themselves may be
 * NULL); entry i receives fp32 [batch*tokens][3*embed_dim] / [batch*tokens][mlp_hidden] of block i. */
int p2v_forward_taps(p2v_plan* plan, const float* images, int batch, const int8_t* bit_config, int n_cfg,
                     float* logits, void* workspace, size_t workspace_bytes, float* const* qkv_out, float* const* fc1_out,
                     void* stream);

/* p2v_forward with the output of EVERY linear layer (ABI 6): what cka_utility.py:26-113 hooks on QConv2d / QLinear when it is given a
 * bit_config.  taps: HOST array of n_cfg device pointers indexed like bit_config (entries may be NULL = skip):
 *   taps[0]            fp32 [batch*patches][embed_dim]           patch-embed convolution output (row b*patches + p: the [B, D, H/P, W/P]
 *                                                                  tensor of the reference, channels last)
 *   taps[1+4i+{0..3}]  fp32 [batch*tokens][3D | D | hidden | D]   qkv / proj / fc1 / fc2 of block i
 *   taps[n_cfg-1]      fp32 [batch][num_classes]                 head output before act_out
 * Every entry holds the QLinear / QConv2d output fmaf(acc, colscale, bias) - one fp32 rounding, the value of p2v_forward_taps' qkv / fc1
 * taps.  qkv and fc1 come from the epilogues of their own launches; proj, fc2, embed and head from one extra fp32-output GEMM each over
 * the layer's int8 input right after the layer's launch.  The logits equal p2v_forward's.  A plan with inv_s_input == 0 (input_quant =
 * False) has no integer patch-embed input: taps[0] != NULL returns P2V_E_UNSUPPORTED there (the other taps work). */
int p2v_forward_linear_taps(p2v_plan* plan, const float* images, int batch, const int8_t* bit_config, int n_cfg,
                            float* logits, void* ws, size_t ws_bytes, float* const* taps, void* stream);

/* ---- uint8 input (additive: no structure, existing entry point or P2V_ABI_VERSION changes; a binding finds it by its symbols) ----------
 * A loader hands over the uint8 crop (what PIL / numpy collate to) instead of the ToTensor + Normalize output.  The normalised value of a
 * pixel depends only on (channel, byte), so the caller passes a LOOKUP TABLE, dev [in_chans][256], built on the host with the loader's own
 * fp32 operations: x = (v / 255.0f - mean[c]) / std[c], two IEEE divisions (data.normalize_uint8 / data.uint8_lut in the Python package).
 *   - plan with an input QAct (inv_s_input > 0): int8 lut[c][v] = clamp(rne(x * inv_s_input), -128, 127), the code k_quantize_patchify
 *     writes for x;
 *   - plan with inv_s_input == 0 (input_quant = False): fp32 lut[c][v] = x, the value the fp32-image convolution reads.
 * The kernels only gather through the table, so the logits equal p2v_forward's on the normalised fp32 batch, bit for bit.  `images`
 * starts on a 4-byte boundary; the table may be anywhere. */
enum { P2V_LAYOUT_NCHW = 0, P2V_LAYOUT_NHWC = 1 };   /* [B][C][H][W] / [B][H][W][C] uint8 */

/* p2v_forward on uint8 images: same workspace (p2v_workspace_bytes), same launch sequence after the input stage, same stop_after
 * numbering (stop_after = 1 leaves the patch matrix in the "patches" buffer).  P2V_E_ARG: null images / lut, unknown layout. */
int p2v_forward_u8(p2v_plan* plan, const uint8_t* images, int layout, const void* lut, int batch, const int8_t* bit_config, int n_cfg,
                   float* logits, void* workspace, size_t workspace_bytes, int stop_after, void* stream);

/* Kernel kinds reported by p2v_forward_profile. */
enum {
  P2V_K_PATCHIFY = 0, P2V_K_GEMM_EMBED = 1, P2V_K_FILL_CLS = 2, P2V_K_LAYERNORM = 3, P2V_K_GEMM_QKV = 4,
  P2V_K_ATTENTION = 5, P2V_K_GEMM_PROJ = 6, P2V_K_GEMM_FC1 = 7, P2V_K_GEMM_FC2 = 8, P2V_K_GEMM_HEAD = 9,
  P2V_K_LN_GEMM_QKV = 10, P2V_K_LN_GEMM_FC1 = 11,  /* LayerNorm fused into the GEMM that consumes it (p2v_ln_gemm_i8) */
  P2V_K_EVENT_GAP = 12     /* not a launch: the last interval of a profile pass, two events with NOTHING between them - what an event pair
                              itself adds to every interval on this stream (subtract it to compare with rocprofv3's kernel durations) */
};

/* Same as p2v_forward, with a hipEvent recorded on `stream` between consecutive launches; synchronises on the
 * last event (measurement only -- never call inside a timed region).  Returns the number of launches (>= 0) or
 * an error; ms_out[i] / kind_out[i] (HOST arrays, max_launches entries) receive the time from launch i to launch
 * i+1 on the stream and the P2V_K_* kind of launch i. */
int p2v_forward_profile(p2v_plan* plan, const float* images, int batch, const int8_t* bit_config, int n_cfg,
                        float* logits, void* workspace, size_t workspace_bytes, void* stream, float* ms_out,
                        int32_t* kind_out, int max_launches);

/* The same measurement for forwards that run CONCURRENTLY on several streams (the batch slices of the default step): _begin enqueues
 * the forward with its events on `stream` and returns at once with a token; _end synchronises on that forward's last event, fills
 * ms_out / kind_out like p2v_forward_profile, frees the token and returns the number of launches.  Begin every slice first, then end
 * them: ms_out[i] is then the duration of launch i WHILE the other streams' kernels run.  Every token must be ended; _end with
 * ms_out == NULL only waits for the forward and frees the token (error paths).  The events of a pass are created before its first
 * launch is enqueued (an event created between two launches would pace the host and the interval would measure the host), and the
 * returned count never exceeds max_launches. */
int p2v_forward_profile_begin(p2v_plan* plan, const float* images, int batch, const int8_t* bit_config, int n_cfg,
                              float* logits, void* workspace, size_t workspace_bytes, void* stream, void** token);
int p2v_forward_profile_end(void* token, float* ms_out, int32_t* kind_out, int max_launches);

/* byte offsets of the named activation buffers inside the workspace for `batch` ("patches", "x", "ln",
 * "qkv", "att", "hid", "cls"); returns <0 for unknown names. */
long long p2v_workspace_view(const p2v_plan* plan, int batch, const char* name);

/* ---- per-operator entry points (unit parity, and the module-level surface) --------------------------- */

/* QAct(qact_input) + im2col for the k=stride=patch QConv2d (vit_fquant.py:705-706, layers.py:55-88):
 * out[b*gh*gw + py*gw + px][c*P*P + i*P + j] = clamp(rne(img[b][c][py*P+i][px*P+j] * inv_s), -128, 127);
 * columns [C*P*P, k_pad) are zeroed. */
int p2v_quantize_patchify(const float* img, int batch, int chans, int height, int width, int patch,
                          float inv_s, int8_t* out, int k_pad, void* stream);

/* p2v_quantize_patchify from uint8 images (layout P2V_LAYOUT_*) through lut_i8 (dev int8 [chans][256], see p2v_forward_u8): byte-equal to
 * it on the normalised fp32 images, padding columns included.  One workgroup per (image, band of `patch` pixel rows); the band and the
 * table are staged in LDS, so chans * 256 + chans * patch^2 bytes must fit 64 KB (P2V_E_UNSUPPORTED beyond). */
int p2v_u8_patchify(const uint8_t* img, int layout, const void* lut_i8, int batch, int chans, int height, int width, int patch,
                    int8_t* out, int k_pad, void* stream);

/* out = epilogue(A[M][K] . W[N][K]^T): int8 MFMA (v_mfma_i32_32x32x32_i8), fp32 epilogue in the
 * reference's operation order.  lda/ldo in elements.  `out` is int8 [M][ldo] except HEAD (fp32 [M][ldo]);
 * when out_codes != NULL the HEAD epilogue also writes the int8 logit codes there ([M][ldo]), and the RESID epilogue the codes of the QAct
 * between the layer and the residual add (attn.qact4 / mlp.qact2 of Swin, attn.qact3 / mlp.qact2 of ViT): q3 = clamp(round((acc *
 * colscale[n] + bias[n]) / s_mid[n])), the first rounding of the RESID formula below, int8 [M][ldo].  A tapped RESID launch runs the generic
 * chain of the tiled kernel whatever resid_tab says (same codes, `out` byte-identical with and without the tap); out and out_codes 16-byte
 * aligned, int8-stored weights (P2V_E_UNSUPPORTED for packed4: p2v_gemm_resid_tap below takes both).  Other epilogues ignore out_codes.
 * K is a multiple of 64 and MAY exceed lda (a width that is not a multiple of 64: the weight columns [width, K) are zero): the
 * contraction then walks into the next row, so (M-1)*lda + K bytes of A must be readable.  ldo >= N.  P2V_E_SHAPE otherwise.
 * REQUANT / GELU / RESID run the tiled kernel, which addresses A and W with 32-bit lane offsets: M*lda + K < 2^32 and
 * round_up(N, 128)*K < 2^32, P2V_E_UNSUPPORTED beyond (the message names the sums); `out` has no such bound.
 * Written: columns [0, N) of rows [0, M) of `out` (and of out_codes, same ldo) - never the columns [N, ldo) - and tap_out as a dense
 * [M][N]; P2V_EPI_EMBED: columns [0, N) of the rows b*(patches+1) + 1 + p, never a class-token row b*(patches+1). */
int p2v_gemm_i8(int epilogue_kind, const int8_t* A, int lda, int M, int K, int N, const p2v_linear* lin,
                const p2v_epilogue* epi, void* out, int ldo, int8_t* out_codes, void* stream);

/* Additive (found by its symbol): p2v_gemm_i8(P2V_EPI_RESID, ..., out_codes) for int8-stored AND packed int4 weights (p2v_linear.packed4),
 * at both tile heights: the ViT / DeiT plans keep their 4-bit layers packed.  Same results and footprint as described above: `out`
 * byte-identical with and without the tap, out_codes = q3, columns [N, ldo) of both never written.  p2v_gemm_i8 itself keeps refusing
 * packed4 for a tapped launch (its callers' contract); the few-rows kernel has no tap (the tiled kernel runs, whatever M). */
int p2v_gemm_resid_tap(const int8_t* A, int lda, int M, int K, int N, const p2v_linear* lin, const p2v_epilogue* epi, int8_t* out, int ldo,
                       int8_t* out_codes, void* stream);

/* Additive (found by its symbol): p2v_gemm_i8(P2V_EPI_EMBED, ...) that also stores the first two roundings of the EMBED chain, taken from
 * the registers that feed the next step: pe_codes = clamp(round(y * inv_s_pe)) (PatchEmbed.qact) and embed_codes = clamp(round(pe_codes *
 * pe_to_embed)) (qact_embed), int8 [rows of out][ldo] in the token layout of `out`: columns [0, N) of the rows b*(patches+1) + 1 + p, never
 * a class-token row, never the columns [N, ldo).  `out` is byte-identical to the launch without the taps.  All three 16-byte aligned. */
int p2v_gemm_embed_tap(const int8_t* A, int lda, int M, int K, int N, const p2v_linear* lin, const p2v_epilogue* epi, int8_t* out, int ldo,
                       int8_t* pe_codes, int8_t* embed_codes, void* stream);

/* rows x C int8 -> rows x C int8; row r of the input starts at x + r*row_stride (lets the final norm
 * touch only the cls rows, vit_fquant.py:766-767).  C: a multiple of 4 up to 4096 (P2V_E_SHAPE beyond, before any launch; see the limits above for the bound
 * on the PTF masks of rows wider than 2048); row_stride and out_stride: independent multiples of 4, out_stride >= C, and beyond 2048 channels
 * row_stride >= C as well (P2V_E_SHAPE: input rows that overlap are taken only at the widths that took them before); bytes
 * [C, out_stride) of an output row and rows >= `rows` are not written. */
int p2v_int_layernorm(const int8_t* x, long long row_stride, int rows, int C, const p2v_ln* ln,
                      int8_t* out, long long out_stride, void* stream);

/* Additive (found by its symbol): p2v_int_layernorm that also writes what a forward hook on the QIntLayerNorm module sees (layers.py:
 * 288-289): tap_out[r][c] = o * out_scale[c] as fp32, o = the rounded integer of the LayerNorm in front of post_mul and of the clamp to int8
 * (|o| may pass 127), out_scale[c] = ln->out_scale[c] where given, else 1 / inv_out[c] (exact for powers of two).  tap_out: dev fp32, dense
 * [rows][C], 16-byte aligned.  `out` is byte-identical to p2v_int_layernorm's, on the generic and on the fast chain, with and without
 * ln->pre.  C up to 2048 (P2V_E_UNSUPPORTED beyond); the other conditions are p2v_int_layernorm's. */
int p2v_int_layernorm_tap(const int8_t* x, long long row_stride, int rows, int C, const p2v_ln* ln,
                          int8_t* out, long long out_stride, float* tap_out, void* stream);

/* p2v_int_layernorm followed by p2v_gemm_i8 (REQUANT or GELU) in ONE launch: norm1 -> qkv -> qact1 and norm2 -> fc1 -> GELU -> qact1
 * (vit_fquant.py:431-434,284-293,307; layers_quant.py:305-316,331-333).  The LayerNorm output codes stay in LDS; ln_out (optional,
 * dev int8 [M][C]) also receives them.  x: dev int8, row r at x + r*row_stride, C channels; lin: weights [n_pad][round_up(C,64)].
 * Reads lin->w_frag (fragment-order weights), not lin->w_codes.  Bit-identical to the two separate calls.  P2V_E_UNSUPPORTED when
 * the shape is not instantiated (C > 384, or the layer's constants do not fit two workgroups per CU) or w_frag is NULL: run the
 * two calls instead. */
int p2v_ln_gemm_i8(int epilogue_kind, const int8_t* x, long long row_stride, int M, int C, const p2v_ln* ln, int N,
                   const p2v_linear* lin, const p2v_epilogue* epi, int8_t* out, int ldo, int8_t* ln_out, void* stream);
/* 1 when p2v_ln_gemm_i8 has an instantiation for this shape (epilogue REQUANT or GELU, C channels, N outputs, cells of the GELU table or
 * 0) in this process (the A/B switch P2V_LN_GEMM=0 turns every shape off), else 0: callers that record launch sequences ask first. */
int p2v_ln_gemm_fusable(int epilogue_kind, int C, int N, int gelu_table_cells);

/* fused attention core on the int8 qkv tensor [batch*tokens][3*heads*head_dim] (layout of
 * qkv.reshape(B,N,3,H,hd), vit_fquant.py:309-315); out int8 [batch*tokens][heads*head_dim].
 * probs_k (optional, dev int8 [batch][heads][tokens][tokens]) receives the log2 softmax exponents
 * (16 = zero) for parity tests. */
int p2v_lis_attention(const int8_t* qkv, int batch, int tokens, int heads, int head_dim, const p2v_attn* at,
                      int8_t* out, int8_t* probs_k, void* stream);
/* (additive: no structure, existing entry point or P2V_ABI_VERSION changes; a binding finds it by its symbol)
 * The same core for the first `query_rows` query tokens of every image only (1 <= query_rows <= tokens; all keys and values take
 * part): what the last block of a ViT needs, whose output is read through the class token alone.  Same layouts and checks as
 * p2v_lis_attention, no probs_k tap.  The kernel works in blocks of 16 query rows: rows 0 .. min(tokens, 16 * ceil(query_rows / 16)) - 1
 * of every image in `out` are written (each with its own, correct values), the rows behind them are not touched: so the resident and
 * the packed kernel.  Where the streaming kernel runs (p2v_attention_kernel) it computes and writes every row. */
int p2v_lis_attention_rows(const int8_t* qkv, int batch, int tokens, int heads, int head_dim, const p2v_attn* at, int query_rows,
                           int8_t* out, void* stream);

/* Additive (found by its symbol): p2v_lis_attention with the two QActs inside the kernel as PITCHED planes, each optional (NULL):
 *   score_codes   the qact_attn1 codes of every real (query, key) pair, int8
 *   probs_k       the log2 softmax exponents (16 = zero), the values of p2v_lis_attention's probs_k
 * both dev int8 [batch][heads][tokens][pitch], 16-byte aligned, pitch >= tokens and a multiple of 16 (rows and images start 16-byte aligned,
 * what p2v_pair_cosine asks for).  Written: columns [0, tokens) of every row; the columns [tokens, pitch) keep the caller's bytes.  The
 * codes are taken from the registers that feed the softmax (the resident kernel: row maximum minus the table offset of the slot), no score
 * is computed twice.  `out` is byte-identical to p2v_lis_attention's.  Same checks as p2v_lis_attention; a tapped launch beyond the resident
 * kernel's token count runs the streaming kernel (p2v_attention_kernel(head_dim, tokens, 1)).  P2V_E_ARG: pitch < tokens, pitch % 16, a
 * misaligned plane - only when a plane is given; with both NULL the call is p2v_lis_attention(..., probs_k = NULL). */
int p2v_lis_attention_taps(const int8_t* qkv, int batch, int tokens, int heads, int head_dim, const p2v_attn* at, int8_t* out,
                           int8_t* score_codes, int8_t* probs_k, int pitch, void* stream);

/* ---- Width of the log-int-softmax (additive: no structure, existing entry point or P2V_ABI_VERSION changes; found by their symbols) ----
 * QIntSoftmax clamps at the width of its own bit type (layers.py:372-375; Config.BIT_TYPE_S, config.py:34-36: uint4, or uint3):
 *     p = 2^-k for k < 2^softmax_bits, else 0,        softmax_bits 3 or 4.
 * The entry points above run at 4.  The *_bits forms take the width; at 4 they write the bytes of the forms above.  A tap plane holds
 * k >= 2^softmax_bits ? 16 : k, so "16 = zero" goes on holding for every reader of such a plane (P2V_COS_LOG2K, P2V_STAT_U8).
 * Any other width: P2V_E_UNSUPPORTED.
 * Range.  The kernels carry the probabilities scaled by 2^-(127 - 2^softmax_bits) and fold the inverse into av_mul (one multiply per
 * output): av_mul * 2^(127 - 2^softmax_bits) has to stay finite, so the accepted range of av_mul (p2v_attn), and of s_q1 / s_q3 (p2v_winattn),
 * is NARROWED at 3 bits: [2^-40, 2^7] instead of [2^-40, 2^15]; beyond it P2V_E_UNSUPPORTED.  (Calibrated models sit many octaves below
 * either bound.)  Every argument and range refusal comes before any launch.
 * Plans: p2v_plan_set_softmax_bits(plan, block, bits) sets the width of one block's attention (4 unless set), in either order with
 * p2v_plan_set_block - both check the block's av_mul against the width's range.  P2V_E_UNSUPPORTED on a plan whose softmax is the table one
 * (p2v_plan_set_float_ops, float_softmax != 0: that softmax has no width), P2V_E_ARG for a block out of range.  Every forward of the plan
 * (taps, DDV stages, statistics, profiling, the class-row last block) runs each block at its width.
 * P2V_OP_WINATTN reads the width from i4, which the kind did not read before: 0 = 4, so earlier records keep their meaning. */
int p2v_lis_attention_bits(const int8_t* qkv, int batch, int tokens, int heads, int head_dim, const p2v_attn* at, int softmax_bits,
                           int8_t* out, int8_t* probs_k, void* stream);
int p2v_lis_attention_rows_bits(const int8_t* qkv, int batch, int tokens, int heads, int head_dim, const p2v_attn* at, int softmax_bits,
                                int query_rows, int8_t* out, void* stream);
int p2v_lis_attention_taps_bits(const int8_t* qkv, int batch, int tokens, int heads, int head_dim, const p2v_attn* at, int softmax_bits,
                                int8_t* out, int8_t* score_codes, int8_t* probs_k, int pitch, void* stream);

/* Swin window attention core (WindowAttention.forward between qact1 and qact3, swin_quant.py:186-217; window partition /
 * cyclic shift / reverse of SwinTransformerBlock.forward, swin_quant.py:366-391, folded into the addressing):
 *   (q*scale) @ k^T -> qact_attn1 -> + qact_table(relative_position_bias_table)[index] -> qact2 -> (+ -100 mask) ->
 *   QIntSoftmax(log-int, uint4, sf = qact2 scale) -> @ v -> qact3.
 * q*scale rounds each element once in fp32 and the dot product over head_dim is exact (fp64), then rounded once.
 * Windows of ws x ws tokens, 1 <= ws <= 12: beyond 12 p2v_window_attention returns P2V_E_SHAPE. */
typedef struct p2v_winattn {
  float s_q1;        /* qact1 scale (pot)                                        */
  float qk_scale;    /* head_dim^-0.5 (swin_quant.py:80)                         */
  float s_attn;      /* qact_attn1 scale (pot)                                   */
  float s_table;     /* qact_table scale (pot)                                   */
  float s_q2;        /* qact2 scale (pot) = the softmax scaling factor           */
  float s_q3;        /* qact3 scale (pot)                                        */
  int32_t x0_int, b_int, c_int; /* I-BERT constants for sf = s_q2 (layers.py:334-351) */
  const int8_t* table_codes;    /* dev [(2*ws-1)^2][heads] codes of qact_table(relative_position_bias_table); 529 rows at ws = 12 */
  const int32_t* win_index;     /* dev [n_windows][ws*ws]: row (within the image) of token p of window w after shift+partition */
  const int8_t* region;         /* dev [n_windows][ws*ws] shifted-window region ids, or NULL (no mask): pairs from different
                                 * regions get -100 (swin_quant.py:325-349)                                                   */
  int32_t ws, n_windows;        /* window side (1 .. 12) and windows per image; ws*ws*n_windows <= tokens_per_image */
  int32_t qkv_stride;           /* bytes between qkv rows (0 = dense: 3*heads*head_dim)                  */
  int32_t out_stride;           /* bytes between out rows (0 = dense: heads*head_dim); lets the next GEMM read K padded to 64.  The kernel writes
                                 * the heads*head_dim codes of a row and NEVER the padding behind them: it keeps the caller's bytes, which
                                 * that GEMM meets with zero weight columns */
} p2v_winattn;

/* qkv int8 [batch][tokens_per_image][3*heads*head_dim] (qact1 codes, natural token order); out int8
 * [batch][tokens_per_image][heads*head_dim] (qact3 codes, natural order).  head_dim must be 32.  probs_k optional:
 * dev int8 [batch][n_windows][heads][N][N] log2 exponents (16 = zero). */
int p2v_window_attention(const int8_t* qkv, int batch, int tokens_per_image, int heads, int head_dim,
                         const p2v_winattn* wa, int8_t* out, int8_t* probs_k, void* stream);

/* Additive (found by its symbol): p2v_window_attention with the three QActs inside the kernel as PITCHED planes, each optional (NULL):
 *   attn1_codes   qact_attn1 codes            qact2_codes   qact2 codes (behind the bias-table add, in front of the -100 mask)
 *   probs_k       log2 softmax exponents (16 = zero), the values of p2v_window_attention's probs_k
 * dev int8 [batch][n_windows][heads][N][pitch], N = ws * ws, 16-byte aligned, pitch >= N and a multiple of 16.  Written: columns [0, N) of
 * every row, nothing else.  `out` is byte-identical to p2v_window_attention's; same checks, both kernels (windows up to 8 x 8 and 9 x 9 ...
 * 12 x 12).  P2V_E_ARG for a bad pitch or a misaligned plane when a plane is given. */
int p2v_window_attention_taps(const int8_t* qkv, int batch, int tokens_per_image, int heads, int head_dim, const p2v_winattn* wa,
                              int8_t* out, int8_t* attn1_codes, int8_t* qact2_codes, int8_t* probs_k, int pitch, void* stream);
/* the two entry points above at a softmax width of 3 or 4 bits (see "Width of the log-int-softmax") */
int p2v_window_attention_bits(const int8_t* qkv, int batch, int tokens_per_image, int heads, int head_dim, const p2v_winattn* wa,
                              int softmax_bits, int8_t* out, int8_t* probs_k, void* stream);
int p2v_window_attention_taps_bits(const int8_t* qkv, int batch, int tokens_per_image, int heads, int head_dim, const p2v_winattn* wa,
                                   int softmax_bits, int8_t* out, int8_t* attn1_codes, int8_t* qact2_codes, int8_t* probs_k, int pitch,
                                   void* stream);

/* PatchMerging.forward gather (swin_quant.py:446-459): x int8 [batch][H*W][C] -> out int8 [batch][(H/2)*(W/2)][4*C] in the
 * reference's channel order x0 (even row, even col), x1 (odd row, even col), x2 (even row, odd col), x3 (odd, odd). */
int p2v_patch_merge_gather(const int8_t* x, int batch, int H, int W, int C, int8_t* out, void* stream);

/* SwinTransformer.forward_features tail (swin_quant.py:806-808): AdaptiveAvgPool1d over the tokens of the fake-quantised
 * qact2 output (codes * s_in, power-of-two s_in: the sum is exact), then qact3: out[b][c] = clamp(round((sum*s_in / tokens) * inv_s_out)). */
int p2v_avgpool_quant(const int8_t* x, int batch, int tokens, int C, float s_in, float inv_s_out, int8_t* out, void* stream);

/* A recorded sequence of the per-operator entry points above, replayed by ONE call: the host-side cost of a forward with a
 * few hundred launches (Swin: ~200) drops to one FFI crossing, and the sequence can be replayed on any stream.  Every record is
 * plain data; pointers are device pointers borrowed for the call.  kind selects which members are read:
 *   P2V_OP_PATCHIFY   in (fp32 images), out; i0 batch, i1 chans, i2 height, i3 width, i4 patch, i5 k_pad; f0 inv_s
 *   P2V_OP_GEMM       in (A), out; epi; M, K, N, lda, ldo; lin; ep
 *   P2V_OP_LAYERNORM  in, out; M rows, N channels, lda / ldo row strides; ln
 *   P2V_OP_WINATTN    in (qkv), out; i0 batch, i1 tokens per image, i2 heads, i3 head_dim; wa
 *   P2V_OP_MERGE      in, out; i0 batch, i1 H, i2 W, i3 C
 *   P2V_OP_AVGPOOL    in, out; i0 batch, i1 tokens, i2 C; f0 s_in, f1 inv_s_out
 *   P2V_OP_LN_GEMM    in (residual-stream codes), out; epi (REQUANT / GELU); M rows, K = C channels of the LayerNorm, N, lda row stride
 *                     of `in`, ldo == N; ln; lin (w_frag required); ep      = p2v_ln_gemm_i8: LayerNorm fused into the GEMM that reads it
 *   (appended, additive - no structure, earlier kind or P2V_ABI_VERSION changes:)
 *   P2V_OP_GEMM, epi == P2V_EPI_RESID: ep.tap_out, read as int8_t*, optionally names the MID-code destination [M][ldo] (p2v_gemm_i8's
 *                     out_codes for RESID); REQUANT / GELU records of P2V_OP_GEMM and P2V_OP_LN_GEMM pass ep.tap_out (fp32 [M][N]) through
 *   P2V_OP_COS        one DDV stage: samples [0, n) of the live buffer `in` against samples [n, 2n) of it.  i0 n, i1 dtype (P2V_COS_*),
 *                     M rows, N cols, lda row stride, i2 | i3 << 32 sample stride (elements; p2v_cos_layer's rules); lin.colscale the
 *                     per-channel scales or NULL; lin.w_codes the stage's record in the device table of p2v_cos_stage_descs (built from
 *                     the same layer); out the partial slots of the whole table.  One launch
 *   P2V_OP_COS_COMBINE  closes the stages of a sequence: in the device table, i1 its stages (>= 1), i0 n, lin.w_codes the partial slots,
 *                     out sums fp64 [stages][n][3].  One launch
 *   P2V_OP_GEMM_F32   in (A), out fp32 [M][ldo] = fmaf(acc, colscale, bias), columns [0, N) only: M, K, N, lda, ldo (N: dense, or a multiple
 *                     of 4 beyond it); lin; in and out 16-byte aligned.  (The public p2v_gemm_i8 refuses this epilogue.)
 *   P2V_OP_WINATTN    optionally names the planes of p2v_window_attention_taps in members the kind did not read before (all NULL / 0 in
 *                     an earlier record: the untapped launch): lin.w_codes the qact_attn1 plane, lin.w_frag the qact2 plane, ep.tap_out the
 *                     exponent plane (all three written as int8_t*), ldo the pitch
 *   P2V_OP_COS        i1 may be P2V_COS_LOG2K (the exponent plane; lin.colscale must be NULL)
 *   P2V_OP_WINATTN_SOFTMAX  p2v_window_softmax_attention: the members of P2V_OP_WINATTN (in, out; i0 batch, i1 tokens per image, i2 heads,
 *                     i3 head_dim; wa), and lin.w_codes - a tap plane of P2V_OP_WINATTN, which an untapped launch does not read - names
 *                     the softmax table (written as const uint32_t*, dev [256]).  The kind has no taps: lin.w_frag, ep.tap_out and ldo
 *                     are not read
 *   P2V_OP_STATS      one stage of the stage statistics (p2v_code_stats below): every sample of the live buffer `in` is reduced into the
 *                     record `out` (initialised by p2v_stats_init, accumulated into).  i0 samples, i1 kind (P2V_STAT_*), M rows, N cols,
 *                     lda row stride, i2 | i3 << 32 sample stride (elements; p2v_stat_layer's rules).  One launch
 *   P2V_OP_WINATTN    i4 the softmax width (3 or 4); 0, the value of every earlier record, means 4
 *   P2V_OP_FLOAT_LAYERNORM  p2v_float_layernorm (at the end of this header; a library that has the kind exports
 *                     p2v_float_layernorm_max_channels): in, out; M rows, N channels, lda / ldo row strides - the members of
 *                     P2V_OP_LAYERNORM - and the constants in members no LayerNorm record reads: f0 s_in, f1 eps, lin.w_codes gamma
 *                     (written as const float*), lin.colscale beta, lin.bias g (dev fp32 [N] each, 16-byte aligned), ep.tap_out the
 *                     optional fp32 tap [M][N] (NULL: none).  `ln` is not read */
enum { P2V_OP_PATCHIFY = 0, P2V_OP_GEMM = 1, P2V_OP_LAYERNORM = 2, P2V_OP_WINATTN = 3, P2V_OP_MERGE = 4, P2V_OP_AVGPOOL = 5, P2V_OP_LN_GEMM = 6,
       P2V_OP_COS = 7, P2V_OP_COS_COMBINE = 8, P2V_OP_GEMM_F32 = 9, P2V_OP_WINATTN_SOFTMAX = 10, P2V_OP_STATS = 11, P2V_OP_FLOAT_LAYERNORM = 12 };
typedef struct p2v_op {
  int32_t kind, epi;
  const void* in;
  void* out;
  int32_t M, K, N, lda, ldo;
  int32_t i0, i1, i2, i3, i4, i5;
  float f0, f1;
  p2v_linear lin;
  p2v_epilogue ep;
  p2v_ln ln;
  p2v_winattn wa;
} p2v_op;

/* run ops[0..n_ops) in order on `stream`; stops at the first error (its status is returned, p2v_last_error names the op). */
int p2v_run_ops(const p2v_op* ops, int n_ops, void* stream);
/* same, with HIP events recorded on `stream` around every op: ms[i] = duration of op i (synchronises the stream). */
int p2v_run_ops_profile(const p2v_op* ops, int n_ops, void* stream, float* ms);

/* UniformQuantizer.forward on an fp32 tensor (uniform.py:50-127, base.py:42-45): fake-quant in place of
 * the eager round/clamp chain.  scale has `n_scale` entries (1 = layer-wise) applied along the channel
 * dimension: element i uses scale[(i / inner) % n_scale].  codes (optional) receives the int8 codes. */
int p2v_fake_quant_f32(const float* x, long long n, const float* scale, int n_scale, long long inner,
                       int lo, int hi, float* out, int8_t* codes, void* stream);

/* Exact GELU -> requant threshold table for inv_s = 2^e, 0 <= e <= 12 (mlp.qact1 scale, layers_quant.py:331-333).
 *   p2v_gelu_table_plan   fills t->k, t->off, t->cells (t->table untouched); P2V_E_UNSUPPORTED when inv_s is not such a power
 *                         of two or the table would exceed 4096 cells (callers then leave table == NULL).
 *   p2v_gelu_table_build  t->table = dev buffer of t->cells * 8 bytes, scratch = dev buffer of p2v_gelu_table_scratch_bytes;
 *                         sweeps EVERY finite fp32 with the fp64 erfc on `stream` and SYNCHRONISES it (one-off, plan building):
 *                         P2V_E_UNSUPPORTED if some cell would need two thresholds.
 *   p2v_gelu_table_check  counts (into *mismatches, dev, zeroed by the caller) the finite fp32 values whose table code
 *                         differs from clamp(rne(RN32(gelu(y)) * inv_s)); asynchronous.                                    */
int p2v_gelu_table_plan(float inv_s, p2v_gelu_tab* t);
size_t p2v_gelu_table_scratch_bytes(int cells);
int p2v_gelu_table_build(float inv_s, const p2v_gelu_tab* t, void* scratch, size_t scratch_bytes, void* stream);
int p2v_gelu_table_check(float inv_s, const p2v_gelu_tab* t, unsigned long long* mismatches, void* stream);

/* correctly-rounded fp32 GELU followed by PoT quantisation (checks the fast path of the GELU epilogue
 * against its own fp64 slow path; flags[0] counts slow-path lanes). */
int p2v_gelu_quant_f32(const float* y, long long n, float inv_s, int8_t* codes, unsigned long long* flags,
                       int force_slow, void* stream);

/* max |fast GELU - fp64 GELU| over `count` consecutive fp32 bit patterns starting at first_bits; *max_err
 * (dev, fp32 bits compared as unsigned) must be zeroed by the caller.  Bound check for the epilogue. */
int p2v_gelu_err_sweep(unsigned first_bits, unsigned count, float* max_err, void* stream);

/* Scheduling aid, no data: enqueues `kernels` (1..64) launches of `workgroups` (1..4096) workgroups of 256 threads (with `lds_bytes`, 0..65536,
 * of LDS each) that wait `usec` (1..1000) microseconds on the device's constant-rate counter.  Two streams whose hardware queues are served
 * concurrently finish two such trains in little more than the time of one (10 x 20 us, 64 workgroups: 0.26 ms); streams whose queues share
 * a dispatch pipe, or that share a queue, take 0.46 - 0.60 ms - and a sliced forward on such a pair runs BELOW the one-stream rate
 * (profiles/r04_stream_pool.txt).  The host side probes candidate side streams with it before the first sliced forward (engine.side_streams). */
int p2v_stream_probe(void* stream, int kernels, int usec, int workgroups, int lds_bytes);

/* ---- CKA model diff (ABI 6): efficient_CKA.MinibatchCKA / DDV_CKA.MinibatchAdvCKA on device ------------------------------------
 * One layer of a minibatch: n rows (images) of F features, row i at x + i * ldx (fp32, device).  y == NULL or y == x: the Gram X X^T
 * (only the upper-triangle tiles are computed and the result is exactly symmetric); else X Y^T (MinibatchAdvCKA's x vs adv_x). */
typedef struct p2v_cka_layer {
  const float* x;      /* dev [n][ldx] */
  const float* y;      /* dev [n][ldy] or NULL */
  long long features;  /* F >= 1 */
  long long ldx, ldy;  /* row strides in floats (>= F) */
} p2v_cka_layer;
#define P2V_CKA_MIN_N 4
#define P2V_CKA_MAX_N 256
#define P2V_CKA_CHUNK 4096    /* features per partial product: the chunking depends on (n, F) only */
size_t p2v_cka_workspace_bytes(const p2v_cka_layer* layers, int n_layers, int n);
/* grams: dev fp32 [n_layers][n][n], per layer the reference's _generate_gram_matrix (efficient_CKA.py:23-39): G = X Y^T with a zero
 * diagonal, means = colsum(G) / (n-2), means -= sum(means) / (2(n-1)), G[i][j] -= means[j] + means[i] (in that order), diagonal
 * zeroed.  Products are exact fp32 MFMA chains over 4096-feature chunks; the chunk partials are combined and centred in fp64 in a
 * fixed order (no atomics): the result is bitwise repeatable.  layers: HOST array (copied to the workspace before the call returns).
 * Three launches on `stream`. */
int p2v_cka_grams(const p2v_cka_layer* layers, int n_layers, int n, float* grams, void* ws, size_t ws_bytes, void* stream);
/* update_state / update_state_across_models: acc[a][b] += <G1[a], G2[b]> over the n*n flattened grams (g1: dev fp32 [l1][n*n],
 * g2: dev fp32 [l2][n*n]); self1[a] += <G1[a], G1[a]>, self2[b] += <G2[b], G2[b]> when non-NULL.  Dot products in fp64, fixed order;
 * dtype 0: acc / self are fp32, 1: fp64 (the accumulator dtype of MinibatchCKA). */
int p2v_hsic_accumulate(const float* g1, int l1, const float* g2, int l2, int n, void* acc, void* self1, void* self2, int dtype,
                        void* stream);

/* ---- DDV model diff (additive: no structure, existing entry point or P2V_ABI_VERSION changes; a binding finds it by its symbols) -----
 * modeldiff_p2.compute_ddv:84-116 takes, per hooked layer and seed sample, the cosine between the layer's activation on a clean input
 * and on its perturbed twin.  One stage of that: n samples of rows x cols elements in `a` and in `b`, sample i at + i * sample_stride,
 * row r at + r * row_stride (both in ELEMENTS); int8 codes or fp32 values.  `scale` (int8 only): per-channel fp32 [cols], the value of an
 * element is scale[c] * code - the PTF scales of the residual stream; NULL: one scale for the tensor, which a cosine does not see.
 * Pointers and strides (in bytes) must be multiples of 16: P2V_E_ARG otherwise. */
/* (additive) P2V_COS_LOG2K: int8 bytes k that stand for the probabilities of the 4-bit log2 softmax, 2^-k for 0 <= k <= 15 and 0 from 16 on
 * (read as unsigned bytes).  The sums are exact integers: every value is 2^(15-k) units of 2^-15, a product at most 2^30, accumulated in
 * int64 through the same tree and splits as P2V_COS_I8, converted once and scaled by 2^-30.  That is exact in fp64 while the integer stays
 * below 2^53: a softmax row's probabilities sum to about 1 (each is at most 1.5 times its exact quotient and at most 1), so sum p^2 <= sum p
 * <= ~1.5 per row and a sample of `rows` rows gives at most ~1.5 * rows * 2^30 - below 2^53 for rows < 2^22, which every plan geometry meets
 * (ViT: rows = heads * tokens <= 64 * 4096 = 2^18; Swin: rows = heads * tokens of the image).  For arbitrary bytes the bound is rows * cols <= 2^23; beyond it the one
 * conversion rounds (rows * cols < 2^33 is refused).  scale must be NULL (P2V_E_ARG otherwise). */
enum { P2V_COS_I8 = 0, P2V_COS_F32 = 1, P2V_COS_LOG2K = 3 };      /* (2 is not an element type: it stays refused, as before) */
typedef struct p2v_cos_layer {
  const void* a;       /* dev, n samples */
  const void* b;       /* dev, n samples */
  const float* scale;  /* dev fp32 [cols] or NULL */
  long long sample_stride, row_stride;   /* elements; row_stride >= cols */
  int32_t rows, cols;  /* >= 1 each */
  int32_t dtype;       /* P2V_COS_I8 / P2V_COS_F32 */
} p2v_cos_layer;
size_t p2v_pair_cosine_workspace_bytes(const p2v_cos_layer* layers, int n_layers, int n);
/* sums: dev fp64 [n_layers][n][3] = sum a.b, sum a.a, sum b.b over the dequantised values of sample i.  int8 without scale: the exact
 * integer sums of the codes (v_dot4_i32_i8 into int64, converted once; rows * cols < 2^39).  int8 with scale: per-channel integer sums,
 * then sum_c (double)s_c^2 * S_c in fp64.  fp32: fp64 products (exact) and sums.  A sample is split over workgroups by (n, rows, cols,
 * dtype) only and the partials are combined in a fixed order, no atomics: bitwise repeatable.  layers: HOST array (copied to the
 * workspace before the call returns); ws 256-byte aligned.  Two launches on `stream`. */
int p2v_pair_cosine(const p2v_cos_layer* layers, int n_layers, int n, double* sums, void* ws, size_t ws_bytes, void* stream);
/* The same reduction as records of a replayed sequence (P2V_OP_COS per stage, one P2V_OP_COS_COMBINE at the end; the op table of p2v_op).
 * p2v_cos_stage_descs checks the layers like p2v_pair_cosine and writes n_layers opaque stage records of p2v_cos_stage_desc_bytes() each to
 * HOST memory; the caller uploads them once (8-byte aligned) and keeps them with the sequence.  Returns the number of partial slots (3 x
 * uint64 each) the stages write, or a negative status. */
size_t p2v_cos_stage_desc_bytes(void);
long long p2v_cos_stage_descs(const p2v_cos_layer* layers, int n_layers, int n, void* host_descs);

/* The quantized model's DDV inside the fused forward.  images: dev fp32 [2n][in_chans][img][img], n clean images then their n perturbed
 * twins; logits: dev fp32 [2n][num_classes], equal to p2v_forward's.  Right after the launch that completes a stage, two small launches
 * reduce rows [0, n*tokens) of the live int8 buffer against rows [n*tokens, 2n*tokens).  Stages, in module order (sums: dev fp64
 * [p2v_ddv_stage_count][n][3]):
 *   qact1                                          "x" after the class-token fill, per-channel scales
 *   blocks.i.attn.qact1 / attn.qact2                "qkv" / "att", one scale each (exact integer sums)
 *   blocks.i.qact2                                  "x" after proj + residual, per-channel scales
 *   blocks.i.mlp.qact1                              "hid" (exact)
 *   blocks.i.qact4                                  "x" after fc2 + residual, per-channel scales
 *   qact2, act_out                                  the class rows after the final norm (exact), the logits (fp32)
 * = 5 * depth + 3.  with_linear != 0 adds the fp32 outputs of blocks.i.attn.qkv / attn.proj / mlp.fc1 / mlp.fc2 (each in front of the
 * QAct that follows it) and of `head` (in front of act_out), 4 * depth + 1 more: every one is written to the ONE buffer tap_scratch
 * (p2v_ddv_tap_scratch_bytes: the largest single tap of 2n images) by the mechanisms of p2v_forward_linear_taps and reduced before the
 * next one overwrites it.  tap_scratch may be NULL when with_linear == 0.  ws: p2v_ddv_workspace_bytes(plan, n) (the forward's
 * workspace of 2n images plus the reduction's partials).  Every row of the last block is computed, as in the tap entry points. */
int p2v_ddv_stage_count(const p2v_plan* plan, int with_linear);
size_t p2v_ddv_workspace_bytes(const p2v_plan* plan, int n);
size_t p2v_ddv_tap_scratch_bytes(const p2v_plan* plan, int n);
int p2v_forward_ddv(p2v_plan* plan, const float* images, int n, const int8_t* bit_config, int n_cfg, float* logits, void* ws,
                    size_t ws_bytes, int with_linear, float* tap_scratch, size_t tap_scratch_bytes, double* sums, void* stream);

/* The stage set (additive; the three functions above are the stage_set = P2V_DDV_STAGES_ENGINE case of these, launch for launch).
 * P2V_DDV_STAGES_FULL serves every hook point of modeldiff_p2.add_hooks but qact_pos (input-independent: its DDV is the constant [1.0]).
 * It adds, in execution order:
 *   qact_input, patch_embed.qact, qact_embed       in front of qact1: the patch matrix (a permutation of the image's codes plus zero columns);
 *                                                  the two mid-code planes of the EMBED launch (p2v_gemm_embed_tap) in "qkv" - patch_embed.qact
 *                                                  over the patch rows [patches][D], qact_embed over [tokens][D] with the constant class row of
 *                                                  p2v_plan_set_embed_tap_cls filled in; one scale each (exact integer sums)
 *   blocks.i.norm1 / norm2                         in front of attn.qkv / mlp.fc1: the LayerNorm's UNCLAMPED integer times out_scale, fp32
 *                                                  (p2v_int_layernorm_tap) - the pair runs unfused: LayerNorm into "ln", then the GEMM
 *   blocks.i.attn.qact3 / mlp.qact2                between attn.proj / mlp.fc2 and qact2 / qact4: the mid codes of the RESID launch
 *                                                  (out_codes of p2v_gemm_i8) in "ln", per-channel scales s_mid
 *   norm                                           in front of qact2: the final norm once more over all 2n * tokens rows (the hook sits in
 *                                                  front of [:, 0]); the class-row launch that feeds the head stays
 * = 4 * depth + 4 more: 9 * depth + 7 stages, 13 * depth + 8 with the linear outputs.  The fp32 LayerNorm values go through tap_scratch (each
 * reduced before the next tap overwrites it; p2v_ddv_tap_scratch_bytes covers them), so FULL needs tap_scratch even with with_linear == 0.
 * The workspace is the same size for both sets; the logits are byte-equal to p2v_forward's.
 * Refused before any launch: an unknown stage_set (P2V_E_ARG); FULL on a plan without an input QAct (inv_s_input == 0: P2V_E_UNSUPPORTED,
 * there is no qact_input stage) or without p2v_plan_set_embed_tap_cls (P2V_E_STATE); FULL with a NULL or short tap_scratch
 * (P2V_E_WORKSPACE). */
enum { P2V_DDV_STAGES_ENGINE = 0, P2V_DDV_STAGES_FULL = 1 };
int p2v_ddv_stage_count_ex(const p2v_plan* plan, int with_linear, int stage_set);
size_t p2v_ddv_workspace_bytes_ex(const p2v_plan* plan, int n, int stage_set);      /* 0 for an unknown stage_set */
int p2v_forward_ddv_ex(p2v_plan* plan, const float* images, int n, const int8_t* bit_config, int n_cfg, float* logits, void* ws,
                       size_t ws_bytes, int with_linear, int stage_set, float* tap_scratch, size_t tap_scratch_bytes, double* sums,
                       void* stream);

/* ---- Scoring of the logits (additive: no structure, existing entry point or P2V_ABI_VERSION changes; a binding finds it by its symbols) --
 * Precision@k and the cross-entropy loss on the device, with a DEFINED tie rule.  The logits are 8-bit codes times a power of two, so the
 * classes of an image share few distinct values and ties at the top-1 / top-5 boundary are common; topk implementations order them
 * differently.  Here: AMONG EQUAL LOGITS THE LOWER CLASS INDEX RANKS FIRST, and the records carry what a result owes to ties.
 *
 * p2v_score_logits: one record per row of logits (dev fp32 [rows][ld], ld >= classes; columns [classes, ld) are padding, never read)
 * against labels (dev int64 [rows]).  With y = labels[r], x = logits[r], j over [0, classes):
 *   ranks[r] = { gt, eq_lo, eq_hi, argmax }  (dev int32 [rows][4])
 *       gt     = #{ j : x_j > x_y }
 *       eq_lo  = #{ j < y : x_j == x_y }        eq_hi = #{ j > y : x_j == x_y }
 *       argmax = the lowest index at which the row maximum occurs
 *   loss[r] = log(sum_j exp((double)x_j - m)) + m - (double)x_y, m the row maximum, all in fp64  (dev fp64 [rows])
 * Invalid labels: a label outside [0, classes) (torch's ignore_index = -100 included) is never used as an index; the row reports
 * gt = -1, eq_lo = eq_hi = 0, its real argmax and loss = 0.  Nothing asserts or traps.
 * One wave per row, fixed reduction order, no atomics: bitwise repeatable.  One launch on `stream`; rows == 0 launches nothing.
 * P2V_E_ARG: null pointer, rows < 0, classes < 1, ld < classes. */
#define P2V_SCORE_MAX_K 8
int p2v_score_logits(const float* logits, long long ld, int rows, int classes, const long long* labels, int32_t* ranks, double* loss,
                     void* stream);
/* Running totals of a validation pass, one SLOT of p2v_score_totals_bytes(n_k) = 8 * (3 + 3 * n_k) bytes in device memory, zeroed by the
 * caller (8-byte aligned; slots may lie back to back).  0: n_k outside 1 ... P2V_SCORE_MAX_K.
 *   int64 n, invalid;  int64 hit[n_k], sure[n_k], possible[n_k];  double loss_sum
 * p2v_score_accumulate folds `rows` records into the slot.  A row with gt < 0 counts in `invalid` only.  A valid row counts in n, adds
 * its loss to loss_sum, and for each k = ks[q] (HOST array, n_k values >= 1):
 *   hit      += gt + eq_lo < k              the defined rule (lower index first among equal logits)
 *   sure     += gt + eq_lo + eq_hi < k      a hit under every tie order
 *   possible += gt < k                      a hit under some tie order
 * so any topk implementation lands in [sure, possible], and sure == possible means that ties decide nothing.
 * One workgroup: thread t adds the losses of rows t, t + 256, ... in ascending order, the 256 partials go through a fixed tree and the
 * result is added to loss_sum; counters are integer sums.  No atomics: the same sequence of batches gives the same bits.  Launches on one
 * stream into one slot are ordered by the stream; the host reads the slot once, at the end of the pass.  rows == 0 launches nothing.
 * P2V_E_ARG: null pointer, rows < 0, n_k outside 1 ... 8, a k < 1, misaligned slot. */
size_t p2v_score_totals_bytes(int n_k);
int p2v_score_accumulate(const int32_t* ranks, const double* loss, int rows, const int* ks, int n_k, void* totals_slot, void* stream);

/* ---- Search-based profiling inputs (additive: no structure, existing entry point or P2V_ABI_VERSION changes; a binding finds it by its
 * symbols) --------------------------------------------------------------------------------------------------------------------------
 * ModelDiff's Algorithm 1 as the reference runs it (dataset_utility.py:193-302), with the state of the search in device memory.  For the
 * logits O [n][classes] (fp32, taken in fp64) of a model on the current inputs and O0 on the seed inputs:
 *   dist(a, b)  = sqrt(sum_k ((double)a_k - (double)b_k)^2)
 *   diversity   = (sum over all n^2 ordered pairs (i, j) of dist(O_i, O_j)) / n^2        np.mean(cdist(O, O)), diagonal zeros included
 *   divergence  = (sum_i dist(O_i, O0_i)) / n
 *   score       = divergence1 * divergence2 * diversity1 * diversity2, multiplied in this order in fp64      (dataset_utility.py:258)
 * An iteration mutates ONE element `pos` of ONE image `idx` by +epsilon ("right", candidate 0) and by -epsilon ("left", candidate 1), so
 * only row idx of O, row and column idx of the distance matrix D and entry idx of the divergence terms g change.
 *
 * The STATE BLOCK (device memory of the caller, 16-byte aligned, p2v_profile_state_bytes(n, classes) bytes; 0 = outside the limits):
 *   double score, one double of padding; per model D [n][n], g [n], rowd [2][n], rowg [2] (fp64; rowd / rowg: the candidates' distances
 *   of the last step); then per model O [n][classes], O0 [n][classes] (fp32, dense).
 * LIMITS: 1 <= n <= P2V_PROFILE_MAX_N, 1 <= classes <= P2V_PROFILE_MAX_CLASSES, 1 <= image_elems <= 2^30.
 *
 * p2v_profile_init        fills the block from the two models' logits of the seed inputs (dev fp32 [n][classes], dense): O = O0 = logits,
 *                         D, g (= 0) and the score (five launches).
 * p2v_profile_candidates  writes image idx of inputs (dev fp32 [n][image_elems]) twice into staging (dev fp32 [2][image_elems]) with
 *                         element pos replaced by x + epsilon (candidate 0) and x - epsilon (candidate 1): fp32 additions, no clipping.
 *                         16-byte copies where source and destination chunk are aligned, scalar otherwise.  One launch.
 * p2v_profile_step        cand1 / cand2 (dev fp32 [2][classes], dense): the logits of model 1 / model 2 on the staging batch.  Launch 1: the
 *                         n distances from each candidate row to the rows of O (0 in the row's own slot) and its divergence term, into
 *                         rowd / rowg.  Launch 2 (one workgroup): per candidate the n^2 positions of D with row and column idx replaced,
 *                         added in one fixed position order, the n entries of g likewise, the score; then the rule of
 *                         dataset_utility.py:292-301 against the stored score (IEEE comparisons):
 *                             right <= score and left <= score: keep (0);  else right > left: take right (1);  else take left (2).
 *                         On 1 / 2 it commits row and column idx of D, g[idx], row idx of O of both models, the score, and copies
 *                         staging[candidate][pos] to inputs[idx][pos].  Always writes trace_row (dev fp64 [4]) = { score_right,
 *                         score_left, decision, score after }.
 * p2v_profile_diversity   the diversity of one logits tensor (dev fp32 [n][ld], ld >= classes) into *out (dev fp64); ws: n * n * 8 bytes
 *                         of device memory, 8-byte aligned.  Two launches.
 * Every distance comes from one device function with one operand and summation order (independent of pointer alignment), and every sum
 * runs over the positions after the substitution - the initial score too.  So a candidate whose two logits rows equal the current rows bit
 * for bit scores BIT-EQUAL to the stored score and the inputs are kept, as the reference's `<=` does (an input-quantised model, epsilon
 * below the input step).  No atomics; results are bitwise repeatable.  A kernel writes the elements of its result and nothing else.
 * Nothing here allocates, frees or synchronises; launches of one search are ordered by the one stream they are enqueued on.
 * P2V_E_ARG: null pointer; state / inputs / staging not 16-byte, trace_row / out / ws not 8-byte, logits / cand not 4-byte aligned; idx
 * outside [0, n), pos outside [0, image_elems).  P2V_E_SHAPE: n, classes, image_elems outside the limits, ld < classes.  P2V_E_WORKSPACE:
 * state_bytes / ws_bytes too small.  All of them before the first HIP call. */
#define P2V_PROFILE_MAX_N 1024
#define P2V_PROFILE_MAX_CLASSES 65536
size_t p2v_profile_state_bytes(int n, int classes);
int p2v_profile_init(void* state, size_t state_bytes, int n, int classes, const float* logits1, const float* logits2, void* stream);
int p2v_profile_candidates(const float* inputs, int n, long long image_elems, int idx, long long pos, float epsilon, float* staging,
                           void* stream);
int p2v_profile_step(void* state, size_t state_bytes, int n, int classes, const float* cand1, const float* cand2, const float* staging,
                     float* inputs, long long image_elems, int idx, long long pos, double* trace_row, void* stream);
int p2v_profile_diversity(const float* logits, long long ld, int n, int classes, double* out, void* ws, size_t ws_bytes, void* stream);

/* ---- DDV stages inside attention (additive: no structure, existing entry point or P2V_ABI_VERSION changes; found by their symbols) ------
 * P2V_DDV_STAGES_ATTN, or-ed onto P2V_DDV_STAGES_ENGINE or P2V_DDV_STAGES_FULL in the three functions below (the _ex functions keep refusing
 * it), adds per block, in module order between attn.qact1 and attn.qact2,
 *   blocks.i.attn.qact_attn1         the int8 score codes of every (query, key) pair           exact integer sums (P2V_COS_I8)
 *   blocks.i.attn.log_int_softmax    the output of QIntSoftmax, probabilities 0 and 2^-k        exact (P2V_COS_LOG2K)
 * = 2 * depth more stages.  The attention launch of a block runs its tapped form (p2v_lis_attention_taps) into attn_scratch - the two planes
 * of the 2n images of ONE block, [2][2n][heads][tokens][pitch] with pitch = round_up(tokens, 16): p2v_ddv_attn_scratch_bytes(plan, n) =
 * 2 * 2n * heads * tokens * pitch bytes - which is reduced right behind the launch and reused by the next block, like tap_scratch.  Only the
 * columns [0, tokens) of a row are written and read: the result does not depend on what the scratch held, nothing outside its dense extent is
 * written.  Without the flag p2v_forward_ddv_ex2 is p2v_forward_ddv_ex, launch for launch (attn_scratch is ignored); with it the logits and
 * the sums of every other stage are byte-identical.  Refused before any launch: the flag with a NULL or misaligned (16 bytes) attn_scratch
 * (P2V_E_ARG) or a short one (P2V_E_WORKSPACE); everything p2v_forward_ddv_ex refuses. */
enum { P2V_DDV_STAGES_ATTN = 2 };
int p2v_ddv_stage_count_ex2(const p2v_plan* plan, int with_linear, int stage_set);
size_t p2v_ddv_attn_scratch_bytes(const p2v_plan* plan, int n);       /* 0: null plan, n outside 1 .. 2^29 */
int p2v_forward_ddv_ex2(p2v_plan* plan, const float* images, int n, const int8_t* bit_config, int n_cfg, float* logits, void* ws,
                        size_t ws_bytes, int with_linear, int stage_set, float* tap_scratch, size_t tap_scratch_bytes, int8_t* attn_scratch,
                        size_t attn_scratch_bytes, double* sums, void* stream);

/* ---- Weight freeze on the device (additive: no structure, existing entry point or P2V_ABI_VERSION changes; found by their symbols) ------
 * p2v_freeze_weights turns the fp32 weights of one layer (dev [N][ldw], ldw >= K, only 4-byte aligned) into the codes of one bit width in
 * one of the layouts a p2v_linear holds:
 *   code[n][k] = clamp(rne(w[n][k] / scale[n_scale == 1 ? 0 : n]), lo, hi)      [-128, 127] at 8 bits, [-8, 7] at 4 bits
 * with an IEEE division and a round to nearest even - torch.round(w / s), for scales that are powers of two and for scales that are not -
 * zero padded to n_pad = round_up(N, 128) rows of k_pad = round_up(K, 64) codes (every code with n >= N or k >= K is 0; nothing there is read).
 *   P2V_W_ROWS_I8    int8 [n_pad][k_pad], row major: p2v_linear.w_codes with packed4 == 0 (bits 8, or 4-bit codes one per byte)
 *   P2V_W_FRAG_I8    the same codes in MFMA-fragment order: p2v_linear.w_frag with packed4 == 0
 *   P2V_W_TILES_P4   the packed int4 tile images, chunk swizzle included: p2v_linear.w_codes with packed4 == 1 (bits 4 only)
 *   P2V_W_FRAG_P4    the packed fragment order: p2v_linear.w_frag with packed4 == 1 (bits 4 only)
 * p2v_freeze_bytes = n_pad * k_pad, half of it for the two packed layouts; 0 for N or K < 1 (or K > 2^30) or an unknown layout.  The call
 * writes exactly these bytes of `out` (dev, 16-byte aligned) and nothing beyond them; it allocates nothing, does not synchronise and is ONE
 * launch on `stream`: one thread per 16 codes of a row, stored as one 16- or 8-byte vector.
 * Refused before any HIP call: P2V_E_ARG for a null pointer (or a misaligned one: w / scale 4 bytes, out 16 bytes); P2V_E_SHAPE for N or
 * K < 1, ldw < K, n_scale not in {1, N}, an unknown layout; P2V_E_BITS for bits not in {4, 8} and for a packed layout with bits = 8;
 * P2V_E_WORKSPACE for out_bytes < p2v_freeze_bytes. */
enum { P2V_W_ROWS_I8 = 0, P2V_W_FRAG_I8 = 1, P2V_W_TILES_P4 = 2, P2V_W_FRAG_P4 = 3 };
size_t p2v_freeze_bytes(int N, int K, int layout);
int p2v_freeze_weights(const float* w, long long ldw, int N, int K, const float* scale, int n_scale, int bits, int layout, void* out,
                       size_t out_bytes, void* stream);

/* ---- Float LayerNorm and float softmax: Config(ptf=False) / Config(lis=False) (additive: no structure, existing entry point or
 *      P2V_ABI_VERSION changes; found by their symbols) -----------------------------------------------------------------------------------
 * The reference's two float operators between int8 codes (QIntLayerNorm in mode 'ln': F.layer_norm, layers.py:241-243; QIntSoftmax with
 * log_i_softmax = False: x.softmax, layers.py:387-395), each followed by a QAct, restated so that no result depends on a summation order.
 *
 * p2v_float_layernorm: a row of C codes q_c under ONE power-of-two input scale s_in.  S1 = sum q, S2 = sum q^2 (exact integers); in fp64,
 * every operation rounded on its own:
 *     var = ((C S2 - S1^2) / (C C)) s_in s_in;   r = 1 / sqrt(var + eps);   y_c = ((((C q_c - S1) / C) s_in) r) gamma_c + beta_c
 *     out_c = clamp(rne(y_c g_c), -128, 127)
 * gamma, beta, g: dev fp32 [C], 16-byte aligned; g_c = 1 / (channel_scale_c * s_out), a power of two (the caller's to guarantee: the kernel
 * multiplies).  tap_out (optional, NULL): dev fp32 dense [rows][C], 16-byte aligned, receives RN32(y_c) - what a hook on the module sees, up
 * to the distance between this expression and the platform's fp32 F.layer_norm.  C: a multiple of 4 in 16 .. P2V_FLOAT_LN_MAX_C (4096; it was
 * 2048 before p2v_float_layernorm_max_channels existed); row_stride / out_stride as p2v_int_layernorm (multiples of 4, out_stride >= C,
 * beyond 2048 channels row_stride >= C: whole rows); bytes [C, out_stride) of an output row are not written.  Everything else is refused
 * before any launch: P2V_E_UNSUPPORTED for a C or stride that is no multiple of 4, P2V_E_SHAPE for C outside 16 .. 4096.
 * With |q| <= 128 and C <= 4096: C S2 <= 2^38, S1^2 <= 2^38 and |C q - S1| < 2^32 - 64-bit integers, numerators exact in fp64.
 * p2v_float_layernorm_max_channels (additive) returns P2V_FLOAT_LN_MAX_C; its presence also tells that p2v_run_ops knows
 * P2V_OP_FLOAT_LAYERNORM.
 *
 * p2v_softmax_attention: p2v_lis_attention's layouts and score requantisation (the qact_attn1 codes c_ij), then
 *     d_ij = max_j c_ij - c_ij in [0, 255];  E_ij = table[d_ij];  num_ic = sum_j E_ij v_jc;  den_i = sum_j E_ij        (exact integers)
 *     out_ic = clamp(rne((double(num_ic) / double(den_i)) av_mul), -128, 127)                                          (one IEEE fp64 division)
 * table: dev uint32 [256], every entry below 2^21 and table[0] > 0 - the caller's to guarantee at the operator (p2v_plan_set_float_block reads
 * the array back once and refuses others with P2V_E_ARG); the plan builds it as min(rne(exp(-s_attn d) 2^21), 2^21 - 1) in fp64 on the host,
 * the kernel never evaluates exp.  av_mul = s_q1 /
 * qact2 scale, a power of two in [2^-40, 2^15].  head_dim 32 or 64, 1 .. P2V_MAX_TOKENS tokens (P2V_E_UNSUPPORTED otherwise).
 * p2v_softmax_attention_taps also writes the score codes as p2v_lis_attention_taps does (pitched plane, columns [0, tokens) only). */
typedef struct p2v_float_ln {
  float s_in;          /* scale of the input codes, a power of two */
  float eps;
  const float* gamma;  /* dev [C] */
  const float* beta;   /* dev [C] */
  const float* g;      /* dev [C] */
} p2v_float_ln;
typedef struct p2v_softmax_attn {
  float s_qkv_sq, qk_scale, inv_s_attn, av_mul;   /* as p2v_attn */
  const uint32_t* table;                          /* dev [256] */
} p2v_softmax_attn;
#define P2V_FLOAT_LN_MAX_C 4096
int p2v_float_layernorm(const int8_t* x, long long row_stride, int rows, int C, const p2v_float_ln* ln, int8_t* out, long long out_stride,
                        float* tap_out, void* stream);
int p2v_float_layernorm_max_channels(void);
int p2v_softmax_attention(const int8_t* qkv, int batch, int tokens, int heads, int head_dim, const p2v_softmax_attn* at, int8_t* out,
                          void* stream);
int p2v_softmax_attention_taps(const int8_t* qkv, int batch, int tokens, int heads, int head_dim, const p2v_softmax_attn* at, int8_t* out,
                               int8_t* score_codes, int pitch, void* stream);
/* The plan side.  p2v_plan_set_float_ops (right after p2v_plan_create) selects per plan the float LayerNorm (float_norm != 0) and / or the
 * table softmax (float_softmax != 0); P2V_E_UNSUPPORTED when the geometry is outside the operators' (float_softmax: head_dim other than 32 /
 * 64, more than P2V_MAX_TOKENS tokens).  p2v_plan_set_float_block carries a block's constants, indexed like p2v_block.ln1 / ln2 (members of a
 * kind the plan does not use are ignored; the arrays stay the caller's); p2v_plan_set_float_head the final norm's (channel scale all ones: g = 1 / qact2 scale).  p2v_block /
 * p2v_plan_set_block / p2v_plan_set_head are still required and unchanged: they carry everything else.  In such a plan the fused
 * LayerNorm+GEMM kernels do not run behind a float LayerNorm, the last block computes every row, and P2V_DDV_STAGES_ATTN is refused
 * (P2V_E_UNSUPPORTED) under the table softmax: its probabilities are not codes. */
typedef struct p2v_float_block {
  p2v_float_ln ln1[2];
  p2v_float_ln ln2[2][2];
  const uint32_t* softmax_table;   /* dev [256] */
} p2v_float_block;
int p2v_plan_set_float_ops(p2v_plan* plan, int float_norm, int float_softmax);
/* (additive) the width of one block's log-int-softmax, 3 or 4 bits (4 unless set): see "Width of the log-int-softmax" above */
int p2v_plan_set_softmax_bits(p2v_plan* plan, int block, int bits);
int p2v_plan_set_float_block(p2v_plan* plan, int block, const p2v_float_block* blk);
int p2v_plan_set_float_head(p2v_plan* plan, const p2v_float_ln* final_ln);

/* Swin plans run ptf = True; lis = False through p2v_window_softmax_attention (additive, found by its symbol): p2v_window_attention up to and
 * including the qact2 codes c_ij (layouts, strides, window addressing, region ids and the output footprint are that entry point's: the
 * padding behind out_stride rows is never written), then, with U_i the keys of query i's shifted-window region (every key of the window
 * when wa->region is NULL; the row's own token is always in it),
 *     m_i = max_{j in U_i} c_ij;  E_ij = table[m_i - c_ij] for j in U_i, 0 for every other key;  num_ic = sum_j E_ij v_jc;  den_i = sum_j E_ij
 *     out_ic = clamp(rne((double(num_ic) / double(den_i)) (s_q1 / s_q3)), -128, 127)                                  (one IEEE fp64 division)
 * A masked key is exactly zero because the reference's -100 lies 100 / s_q2 >= 400 codes below every key of U_i and exp(-(100 - 255 s_q2)) 2^21
 * rounds to 0: that needs s_q2 <= 2^-2.  table: dev uint32 [256] with p2v_softmax_attention's entry rules (every entry below 2^21,
 * table[0] > 0; the plan builds min(rne(exp(-s_q2 d) 2^21), 2^21 - 1) in fp64 on the host).  wa->x0_int / b_int / c_int are ignored.
 * P2V_E_UNSUPPORTED: head_dim other than 32, s_q2 > 2^-2, s_q1 / s_q3 outside [2^-40, 2^15] or a scale that is no power of two;
 * P2V_E_SHAPE: ws outside 1 .. 12, windows beyond the token count, bad strides; P2V_E_ARG: a null pointer, qkv not 16-byte or out / table /
 * win_index not 4-byte aligned.  All before any launch.  Config(ptf=False) of a Swin model records P2V_OP_FLOAT_LAYERNORM at every
 * LayerNorm (up to 3072 channels: the PatchMerging norm of Swin-L); it composes with either window attention. */
int p2v_window_softmax_attention(const int8_t* qkv, int batch, int tokens_per_image, int heads, int head_dim, const p2v_winattn* wa,
                                 const uint32_t* table, int8_t* out, void* stream);

/* ---- Stage statistics (additive: no structure, existing entry point or P2V_ABI_VERSION changes; a binding finds it by its symbols) -----
 * Which part of its code range a stage uses: one RECORD per stage, reduced over every sample and row of a strided plane, per column.
 * One plane (the addressing of p2v_cos_layer with one operand): `samples` samples of rows x cols elements, sample i at + i * sample_stride,
 * row r at + r * row_stride (both in ELEMENTS, row_stride >= cols; only columns [0, cols) of a row are read).  Element kinds:
 *   P2V_STAT_I8    signed codes                                                     histogram bin = code + 128
 *   P2V_STAT_U8    unsigned bytes (the exponents k of the log2 softmax, 16 ... 255 = probability 0)     bin = the byte
 *   P2V_STAT_F32   fp32 values (layer outputs, LayerNorm values, logits)            bin = the biased exponent field (bits >> 23) & 255
 * The record, p2v_stats_bytes(cols) = 2080 + 24 * cols bytes rounded up to 16, 16-byte aligned, in device memory:
 *   int64 hist[256];  int64 count;  int64 nonfinite[3] (NaN, +Inf, -Inf; zero for the integer kinds)
 *   lo[cols], hi[cols]      int32 for the integer kinds; for F32 the fp32 VALUE, over the finite elements only, in the total order of the
 *                           sign-magnitude key (-0 < +0).  A column without a finite element keeps lo = +Inf, hi = -Inf (integer kinds
 *                           without an element: INT32_MAX, INT32_MIN)
 *   int64 sum[cols], sumsq[cols]     the integer kinds only; F32 leaves them zero (a float sum would depend on the order)
 * p2v_stats_init writes the empty record (one launch); every later reduction ACCUMULATES into it, so one record serves any number of
 * batches.  All quantities are integers or order-independent extrema: the result is defined exactly and is bitwise repeatable whatever the
 * launch geometry.  The kernel keeps per-lane extrema and sums in registers and a histogram per wave in LDS, combines them per workgroup in
 * LDS and adds the workgroup's result with integer atomics (a workgroup visits at most 2^16 rows of at most 1024 columns, so no 32-bit
 * counter of it can overflow).  16-byte loads where a column group is whole and base and strides are 16-byte aligned, scalar loads otherwise.
 * p2v_code_stats: layers is a HOST array, records[l] the record of layer l; one launch per layer on `stream`; a layer with rows == 0 or
 * samples == 0 launches nothing.  ws / ws_bytes are reserved (the atomics form needs no workspace; NULL / 0).
 * P2V_E_ARG: null pointer, unknown dtype, row_stride < cols, negative strides or counts, base or strides (in bytes) no multiples of 16,
 * a record that is not 16-byte aligned; P2V_E_SHAPE: cols < 1; P2V_E_WORKSPACE: p2v_stats_init with bytes < p2v_stats_bytes(cols);
 * P2V_E_UNSUPPORTED: samples * rows >= 2^31.  All before any launch. */
enum { P2V_STAT_I8 = 0, P2V_STAT_F32 = 1, P2V_STAT_U8 = 2 };
typedef struct p2v_stat_layer {
  const void* base;    /* dev */
  long long sample_stride, row_stride;   /* elements; row_stride >= cols */
  int32_t samples, rows, cols;           /* samples, rows >= 0; cols >= 1 */
  int32_t dtype;       /* P2V_STAT_* */
} p2v_stat_layer;
size_t p2v_stats_bytes(int cols);        /* 0 for cols < 1 */
int p2v_stats_init(void* out, size_t bytes, int dtype, int cols, void* stream);
int p2v_code_stats(const p2v_stat_layer* layers, int n_layers, void* const* records, void* ws, size_t ws_bytes, void* stream);

/* The statistics of every stage inside the fused forward: p2v_forward_ddv_ex2's launch sequence, stage sets (P2V_DDV_STAGES_ENGINE / _FULL,
 * optionally | P2V_DDV_STAGES_ATTN), stage order and refusals, with two differences: `batch` is any batch >= 1 (no pairs), and right after the
 * launch that completes a stage ONE launch reduces all `batch` samples of the live buffer into the stage's record.  The attention stages are
 * attn.qact_attn1 (I8) and attn.log_int_softmax (U8: the exponents k); attn.qact3 / mlp.qact2 are their codes (I8), the s_mid scales are in
 * the layout; qact_input covers the real in_chans * patch^2 columns of the patch matrix, not the zero columns up to k_pad.  Every row of the
 * last block is computed and the logits equal p2v_forward's.
 *   p2v_forward_stats_bytes    bytes of the records of all stages, back to back in stage order (0: refused)
 *   p2v_forward_stats_layout   per stage k < max_stages the byte offset of its record, its cols, its kind (P2V_STAT_*) and its per-channel
 *                              scales (dev fp32 [cols], or NULL: one scale for the tensor); any array may be NULL.  Returns the number of
 *                              stages (= p2v_ddv_stage_count_ex2) or a negative status.  Both run the forward's own sequence with no launch
 *                              made, so they cannot disagree with it.
 * The caller initialises every record once (p2v_stats_init) and may run any number of batches into them.  ws: p2v_workspace_bytes(plan,
 * batch); tap_scratch / attn_scratch: p2v_ddv_tap_scratch_bytes / p2v_ddv_attn_scratch_bytes of n = (batch + 1) / 2 pairs, needed as in the
 * DDV call (tap_scratch for with_linear or FULL, attn_scratch for the flag).  Refusals before any launch: those of p2v_forward_ddv_ex2 (the
 * flag under the float softmax P2V_E_UNSUPPORTED, FULL on an input_quant = False plan P2V_E_UNSUPPORTED), stats not 16-byte aligned
 * (P2V_E_ARG); a stats arena shorter than p2v_forward_stats_bytes is refused (P2V_E_WORKSPACE) at the first record that does not fit. */
size_t p2v_forward_stats_bytes(const p2v_plan* plan, int with_linear, int stage_set);
int p2v_forward_stats_layout(const p2v_plan* plan, int with_linear, int stage_set, int max_stages, long long* offsets, int32_t* cols,
                             int32_t* kinds, const float** scales);
int p2v_forward_stats(p2v_plan* plan, const float* images, int batch, const int8_t* bit_config, int n_cfg, float* logits, void* ws,
                      size_t ws_bytes, int with_linear, int stage_set, float* tap_scratch, size_t tap_scratch_bytes, int8_t* attn_scratch,
                      size_t attn_scratch_bytes, void* stats, size_t stats_bytes, void* stream);

/* ---- Stage Grams: CKA over the DDV stage list (additive: no structure, existing entry point or P2V_ABI_VERSION changes) ---------------
 * efficient_CKA.MinibatchCKA / DDV_CKA.MinibatchAdvCKA take Gram matrices over hooked activations.  A STAGE is n samples (images) of
 * rows x cols elements in the addressing of p2v_cos_layer: sample i at + i * sample_stride, row r at + r * row_stride (both in ELEMENTS,
 * row_stride >= cols; only columns [0, cols) of a row are read).  The raw Gram of a stage is G[i][j] = sum_{r,c} v_i[r][c] * v_j[r][c],
 * fp64 [n][n], with a `unit` such that the stage's values are v * unit:
 *   P2V_GRAM_I8, shift == NULL   v = code.  G is the exact integer sum, returned as an (integer-valued) fp64.  unit = the stage's one scale.
 *   P2V_GRAM_I8, shift != NULL   per-channel scales s_c = unit * 2^m_c with unit = min_c s_c (the PTF streams qact1 / qact2 / qact4 and the
 *                                mid codes attn.qact3 / mlp.qact2: m_c in {0, 1, 2, 3}; a ptf = False plan repeats one scale, m_c = 0).
 *                                v = code * 2^m_c with m_c = shift[c] (dev bytes [cols], 16-byte aligned; the low two bits are used).  G is
 *                                again the exact integer sum.  The fp32 value a hook on the QAct sees is RN(code * s_c): it differs from
 *                                v * unit by at most one fp32 rounding per element, and CKA does not depend on unit at all.
 *   P2V_GRAM_F32                 v = the fp32 value, unit = 1, shift must be NULL: the chunked exact-product fp32 MFMA partials and the
 *                                fixed-order fp64 combination of p2v_cka_grams (the same two launches), stored uncentred.  As there, the
 *                                DIAGONAL IS ZERO (the Gram rule discards it before anything reads it).  Rows must be dense
 *                                (row_stride == cols, or rows == 1): P2V_E_UNSUPPORTED otherwise.
 * G is exactly symmetric: the 32 x 32 tiles ti <= tj are computed, the rest is their mirror.  Integer stages are exact while |G| < 2^53
 * (always for one-scale codes: rows * cols * 2^14 < 2^45); rows * cols >= 2^31 is refused before any launch.  Integer kernel: one workgroup
 * per (tile, chunk of P2V_GRAM_CHUNK features) on v_mfma_i32_32x32x32_i8, int32 within a chunk (at most 2^13 features * 2^14 = 2^27;
 * shifted stages split code * 4^m into two byte planes, products at most 2^13), int64 partials, a second launch adds them in chunk order and
 * converts once.  No atomics, fixed order: bitwise repeatable; the splitting depends on (n, rows, cols, dtype) only.
 * p2v_code_grams: layers is a HOST array (used before the call returns), grams dev fp64 [n_layers][n][n] (8-byte aligned), 1 <= n <=
 * P2V_GRAM_MAX_N (any n: edge tiles read and write nothing outside the stage and G); base pointers and shift 16-byte aligned (strides are
 * free: 16-byte loads where base and strides allow them, a scalar tail otherwise); ws 256-byte aligned, p2v_code_grams_workspace_bytes
 * (0: refused).  Two launches per layer on `stream` (fp32: a descriptor copy and two).  Refusals, all before the first HIP call: P2V_E_ARG
 * (null / misaligned pointer, unknown dtype, row_stride < cols, negative sample_stride, shift on an fp32 stage), P2V_E_SHAPE (n, rows,
 * cols < 1, n > P2V_GRAM_MAX_N), P2V_E_UNSUPPORTED (rows * cols >= 2^31, strided fp32 rows), P2V_E_WORKSPACE. */
enum { P2V_GRAM_I8 = 0, P2V_GRAM_F32 = 1 };
typedef struct p2v_gram_layer {
  const void* base;      /* dev, n samples */
  const uint8_t* shift;  /* dev bytes [cols] (int8 only) or NULL */
  long long sample_stride, row_stride;   /* elements; row_stride >= cols */
  int32_t rows, cols;    /* >= 1 each */
  int32_t dtype;         /* P2V_GRAM_* */
} p2v_gram_layer;
#define P2V_GRAM_MAX_N 512
#define P2V_GRAM_CHUNK 8192   /* features per int32 partial sum: 2^13 * 2^14 = 2^27 < 2^31 */
size_t p2v_code_grams_workspace_bytes(const p2v_gram_layer* layers, int n_layers, int n);
int p2v_code_grams(const p2v_gram_layer* layers, int n_layers, int n, double* grams, void* ws, size_t ws_bytes, void* stream);
/* The centring rule of p2v_cka_grams (fp64 centring, fp32 store) on given raw Grams: entry (i, j) of layer l is raw[l * layer_stride +
 * i * pitch + j] (fp64, strides in elements, pitch >= n); grams dev fp32 [n_layers][n][n].  The diagonal of raw is not read (it counts as
 * zero).  With pitch = 2n and raw + n, the off-diagonal n x n block of a 2n x 2n Gram is centred as the X Y^T form - MinibatchAdvCKA's
 * X X_adv^T.  P2V_CKA_MIN_N <= n <= P2V_GRAM_MAX_N.  One launch. */
int p2v_cka_centre(const double* raw, long long pitch, long long layer_stride, int n_layers, int n, float* grams, void* stream);
/* Once per plan, after every block and the embed stage are set (it synchronises, like the other plan setters): derives shift[c] and unit
 * of every per-channel stage scale vector of the plan - the embed s_next, per block proj_epi.s_mid / s_next and fc2_epi.s_mid / s_next -
 * into device bytes the plan owns.  P2V_E_UNSUPPORTED: a vector whose ratios s_c / min_c s_c are not all in {1, 2, 4, 8}; P2V_E_STATE: an
 * incomplete plan. */
int p2v_plan_prepare_grams(p2v_plan* plan);
/* The raw Grams of every stage inside the fused forward: p2v_forward_stats's launch sequence, stage order and scratch rules, with `batch`
 * images (1 ... P2V_GRAM_MAX_N, no pairs) and with_linear / stage_set in {P2V_DDV_STAGES_ENGINE, P2V_DDV_STAGES_FULL} as in
 * p2v_forward_ddv_ex; right after the launch that completes a stage its Gram over all `batch` samples is taken from the live buffer.
 * grams: dev fp64 [stages][batch][batch]; units: dev fp64 [stages] - min_c s_c of a per-channel stage, 1 of an fp32 stage, and 0 for a
 * one-scale int8 stage, whose scale the stage sites do not carry (the layout reports scales == NULL for it; the caller holds the scale).
 * Every row of the last block is computed, as in the tap entry points, and the logits are byte-equal to p2v_forward's.
 *   p2v_forward_grams_stage_count   = p2v_ddv_stage_count_ex
 *   p2v_forward_grams_bytes         the workspace: the forward's of `batch` images plus the partials of the largest stage (0: refused)
 *   p2v_forward_grams_layout        per stage k < max_stages its rows, cols, kind (P2V_GRAM_*) and per-channel scales (dev fp32 [cols] or
 *                                   NULL); any array may be NULL.  Returns the number of stages or a negative status.  It runs the
 *                                   forward's own sequence with no launch made.
 * Refusals before any launch: P2V_DDV_STAGES_ATTN (P2V_E_UNSUPPORTED: the exponent planes are no byte codes), a plan without
 * p2v_plan_prepare_grams (P2V_E_STATE), those of p2v_forward_stats, a short ws or tap_scratch (P2V_E_WORKSPACE), grams_bytes < stages *
 * batch^2 * 8 or units_bytes < stages * 8 (P2V_E_WORKSPACE). */
int p2v_forward_grams_stage_count(const p2v_plan* plan, int with_linear, int stage_set);
size_t p2v_forward_grams_bytes(const p2v_plan* plan, int batch, int with_linear, int stage_set);
int p2v_forward_grams_layout(const p2v_plan* plan, int with_linear, int stage_set, int max_stages, int32_t* rows, int32_t* cols,
                             int32_t* kinds, const float** scales);
int p2v_forward_grams(p2v_plan* plan, const float* images, int batch, const int8_t* bit_config, int n_cfg, float* logits, void* ws,
                      size_t ws_bytes, int with_linear, int stage_set, float* tap_scratch, size_t tap_scratch_bytes, double* grams,
                      size_t grams_bytes, double* units, size_t units_bytes, void* stream);

/* ---- Patch-similarity entropy of PSAQ-ViT's data generator and its gradient (generate_data.py:102-113, 128-134; utils/kde.py:87-96) ----
 * av: dev fp32, contiguous [images * groups][heads][tokens][head_dim] - one block's attn @ v before the transpose; groups = windows per image
 * (1 for ViT / DeiT).  Per group: a = mean over heads, row 0 dropped (T = tokens - 1 rows), S = cosine similarity of every pair of rows
 * (each row divided by max(|row|, 1e-8), diagonal computed).  lo / hi = min / max of S over the WHOLE call (constants of the
 * differentiation), x_k = linspace(lo, hi, 10).  Per image over its n = groups * T^2 similarities: p_k = (c / n) sum_m exp(-(x_k - s_m)^2 /
 * (2 h^2)), h = 0.01, c = 1 / sqrt(2 pi h^2); q = p + 1e-4; E_b = trapezoid rule of -q ln q over x.  value_out (dev fp64 [1]) = mean_b E_b;
 * grad_out (dev fp32, the shape of av) = d value / d av, row 0 of every group exactly zero, every head the same slice.  lo == hi gives 0
 * and zeros.  The point sums and the trapezoid are fp64, the products run on the exact-fp32 MFMA, nothing is accumulated with atomics and
 * nothing synchronises: six launches on `stream`, the same bytes on every run.  The workspace (p2v_psaq_workspace_bytes, 256-byte aligned)
 * holds S - images * groups * T * T floats - plus the normalised rows and the partials.
 * P2V_E_SHAPE before any launch: images / groups / heads < 1, T outside 2 ... 1024, head_dim no multiple of 4 in 4 ... 128 (the query
 * returns 0 for these); P2V_E_ARG: a null pointer, av / grad_out not 16-byte, value_out not 8-byte, workspace not 256-byte aligned. */
size_t p2v_psaq_workspace_bytes(int images, int groups, int heads, int tokens, int head_dim);
int p2v_patch_similarity_entropy(const float* av, int images, int groups, int heads, int tokens, int head_dim, void* workspace,
                                 double* value_out, float* grad_out, void* stream);

/* ---- Hutchinson trace bookkeeping around torch's double backward (pyhessian/hessian.py:163-211) ----
 * The Hessian-vector product stays autograd's; these entry points make the probe vectors of all selected tensors in one launch, take
 * v . Hv of all of them in two, and keep every layer's stopping rule on the device.  `segs` is a HOST array, read during the call: up to
 * 64 segments go into one launch, whose table travels as the kernel argument, so nothing is uploaded, nothing synchronises and a graph
 * capture records the call.  Segment pointers are device fp32, 4-byte aligned; a start or length off the 16-byte grid costs scalar
 * accesses at the two ends only.  Nothing outside [ptr, ptr + n) is touched.
 *
 * The generator.  splitmix64(x): x += 0x9E3779B97F4A7C15; z = x; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) *
 * 0x94D049BB133111EB; return z ^ z >> 31 (mod 2^64).  key(seed, layer, probe) = splitmix64(splitmix64(splitmix64(seed) ^ layer) ^
 * probe), layer as an unsigned 32-bit value; element e of the stream is +1.0f when bit e % 64 of splitmix64(key + e / 64) is set, else
 * -1.0f.  A segment's values depend on (seed, layer, probe, e) alone, not on its address or on the other segments of the call.
 *
 * P2V_E_ARG before any HIP call: n_segs outside 1 ... 65536, a null or misaligned pointer, n outside 1 ... 2^31 - 1, probe outside
 * 0 ... max_iter - 1, tol not a number; P2V_E_WORKSPACE: ws / state smaller than the query says. */
typedef struct {
  float* ptr;
  long long n;
  int32_t layer;
} p2v_seg;
typedef struct {
  const float* a;
  const float* b;
  long long n;
} p2v_seg2;
int p2v_rademacher_fill(const p2v_seg* segs, int n_segs, uint64_t seed, uint64_t probe, void* stream);
/* out (dev fp64 [n_segs]): out[s] = sum_e (double)a[e] * (double)b[e] of segment s.  Every product is exact; a workgroup adds 4096 of
 * them in a fixed order into one fp64 partial in ws (p2v_group_dot_workspace_bytes, 8-byte aligned; 0 = refused), a second launch adds a
 * segment's partials in a fixed order.  No floating-point atomics: two runs give the same bytes; NaN and Inf propagate. */
size_t p2v_group_dot_workspace_bytes(const p2v_seg2* segs, int n_segs);
int p2v_group_dot(const p2v_seg2* segs, int n_segs, double* out, void* ws, size_t ws_bytes, void* stream);
/* One probe of all layers: the group dot into record[probe][0 .. n_segs) (dev fp64 [max_iter][n_segs]), then, one thread per layer, the
 * stopping rule: sum += value; mean = sum / (probe + 1); if |mean - trace| / (|trace| + 1e-6) < tol the layer is done and keeps `trace`
 * (the PREVIOUS prefix mean), else trace = mean.  A finished layer ignores later values.  Call with probe = 0, 1, 2, ... in order.
 * state (dev, 8-byte aligned, p2v_hutchinson_state_bytes(n_segs) bytes, cleared by p2v_hutchinson_init):
 *   int32 running (layers not done - the one word a host needs to poll), int32 n_layers, 8 bytes unused; then per layer 32 bytes:
 *   fp64 sum, fp64 trace, int32 probes (consumed; stop index + 1 once done), int32 done, int32 converged, 4 bytes unused. */
size_t p2v_hutchinson_state_bytes(int n_segs);
int p2v_hutchinson_init(void* state, size_t state_bytes, int n_segs, void* stream);
int p2v_hutchinson_step(const p2v_seg2* segs, int n_segs, int probe, int max_iter, double tol, double* record, void* state,
                        size_t state_bytes, void* ws, size_t ws_bytes, void* stream);

/* ---- Many bit lists in one call (additive: no structure, existing entry point or P2V_ABI_VERSION changes; found by their symbols) --------
 * p2v_forward for n_lists bit lists over the same images, sharing what the lists have in common.  bit_configs: HOST int8
 * [n_lists][n_cfg], read when the call is made; logits: dev fp32 [n_lists][batch][classes].  logits[l] is byte-equal to what
 * p2v_forward(plan, images, batch, bit_configs[l], ..., stop_after = -1) writes, for every l in the caller's order, repeated lists
 * included (computed once, their logits copied).
 *
 * Between the blocks of the forward only the residual stream "x" (int8 [batch * tokens][embed_dim]) carries state, and the engine is
 * integer-exact, so a forward resumed from a saved x equals a fresh one.  The lists form a prefix tree of depth + 2 levels: level 0 is
 * keyed by the stem's entry cfg[0], level 1 + i by the four entries of block i, the tail runs the final norm once per distinct block
 * prefix and one head GEMM per distinct cfg[n_cfg - 1] under it.  The tree is walked depth first, children in order of first appearance
 * in the caller's array; every node's launches run once.  A node with c > 1 children saves x once into the snapshot slot of its depth
 * (hipMemcpyAsync device to device on `stream`, batch * tokens * embed_dim bytes) and restores it in front of children 2 ... c.  The root
 * needs none (the stem writes every row of x), nor does the tail (it writes none).  The class-row shortcut of the last block ("cls_rows")
 * applies as in p2v_forward: it writes the class rows of x, which the restore puts back.
 *
 * Workspace: p2v_forward_many_bytes = p2v_workspace_bytes(plan, batch) plus `snapshots` slots of x, each rounded up to 256 bytes;
 * snapshots = the largest number of branching nodes on one root-to-leaf path (0: refused).  Nothing outside [ws, ws + bytes) and logits
 * is written.  No allocation, synchronisation or read-back: both calls can be recorded into a HIP graph (kernels and device-to-device
 * copies on `stream`).  A plan with float operators (p2v_plan_set_float_ops) runs as in p2v_forward.
 *
 * p2v_forward_many_plan is the same walk with nothing enqueued and makes no HIP call; it needs the plan's geometry only.  It returns the
 * numbers of stem runs, block runs, final norms, head GEMMs, copies of x (saves + restores) and snapshot slots; an output pointer may be
 * NULL.  A loop of p2v_forward runs n_lists stems, n_lists * depth blocks, n_lists norms and heads.
 *
 * Refused before any HIP call, the message naming the entry point: P2V_E_ARG (null argument; the image checks of p2v_forward_u8),
 * P2V_E_SHAPE (batch < 1, n_lists outside 1 ... P2V_MANY_MAX_LISTS), P2V_E_BITS (n_cfg is not the plan's, an entry not in {4, 8}),
 * per list what p2v_forward refuses with the same status (P2V_E_STATE: a layer without weights of that width, an incomplete plan),
 * P2V_E_WORKSPACE (ws_bytes < p2v_forward_many_bytes). */
#define P2V_MANY_MAX_LISTS 4096
int p2v_forward_many(p2v_plan* plan, const float* images, int batch, const int8_t* bit_configs, int n_lists, int n_cfg, float* logits,
                     void* ws, size_t ws_bytes, void* stream);
int p2v_forward_many_u8(p2v_plan* plan, const uint8_t* images, int layout, const void* lut, int batch, const int8_t* bit_configs,
                        int n_lists, int n_cfg, float* logits, void* ws, size_t ws_bytes, void* stream);
size_t p2v_forward_many_bytes(const p2v_plan* plan, int batch, const int8_t* bit_configs, int n_lists, int n_cfg);
int p2v_forward_many_plan(const p2v_plan* plan, const int8_t* bit_configs, int n_lists, int n_cfg, int* stems, int* blocks, int* norms,
                          int* heads, int* copies, int* snapshots);

const char* p2v_last_error(void);
int p2v_abi_version(void);

/* Scheduling / A-B switches of the process (also read once from the environment: P2V_LN_GEMM, P2V_LN_GEMM_V, P2V_LN_GENERIC,
 * P2V_LN_ROWS, P2V_ATTN_WAVES, P2V_GEMM_TILE, P2V_RESID_PRE, P2V_LN_PRE, P2V_ATTN_STREAM, P2V_ATTN_PACKED, P2V_GEMM_ROWS, P2V_CLS_ROWS, P2V_LN_GEMM_LEAN).  None of them changes a result - every variant is
 * bit-identical and is driven through this call by the parity tests (profiles/r04_alt_paths.txt: the whole GPU suite on the alternatives):
 *   "ln_gemm" 0/1 (fuse LayerNorm into qkv / fc1), "ln_gemm_version" 1/2/3 (round-2 4-wave / pipelined 4-wave (default) / 8-wave fused kernel),
 *   "ln_gemm_lean" 0/1 (default 1: the pipelined 4-wave kernel runs its lean LayerNorm phase where a launch has pre-folded constants,
 *   C = 64 * k-tiles and no LayerNorm output; 0: the general phase everywhere),
 *   "ln_generic" 0/1 (generic LayerNorm chain), "ln_rows" 1..64, "attn_waves" 4..8,
 *   "gemm_tile" 0/128/256 (tile height of the layer GEMMs; 0 = 256 rows when the grid still fills the chip),
 *   "resid_pre" 0/1 (use p2v_epilogue.resid_tab), "ln_pre" 0/1 (use p2v_ln.pre), "attn_stream" 0/1 (streaming attention kernel everywhere),
 *   "attn_packed" 0/1, nothing else (default 1; 0: beyond the resident kernel's token count every launch takes the streaming kernel),
 *   "cls_rows" 0/1 (default 1: p2v_forward / p2v_forward_u8 / p2v_forward_profile* with stop_after = -1 run the last block behind its qkv
 *   GEMM on the class-token rows only - one query row per (image, head), then proj, norm2, fc1, fc2 on `batch` rows; the logits do not
 *   depend on the other rows.  Consequence: after such a call the workspace views "x", "att", "hid" and "ln" hold the LAST block's values
 *   only where the logits need them (class rows of "x" / "att", the first `batch` rows of "hid" / "ln"); stop_after >= 0, p2v_forward_taps
 *   and p2v_forward_linear_taps compute every row as before and are the way to read full buffers),
 *   "gemm_rows" 0/1/2 (the few-rows GEMM kernel, parallel over N and K instead of M: 0 = where the forward asks for it, i.e. the class rows
 *   above; 1 = every REQUANT / GELU / RESID GEMM, also through p2v_gemm_i8 and p2v_run_ops; 2 = never.  An explicit "gemm_tile" of 128 or 256
 *   always means the tiled kernel). */
int p2v_set_tuning(const char* name, int value);

#ifdef __cplusplus
}
#endif
#endif /* P2VIT_H */
