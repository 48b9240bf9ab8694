// p2vit_capi.cpp -- extern "C" surface of libp2vit_hip.so (see include/p2vit.h).
//
// The plan object is the frozen integer state the reference keeps in Python attributes after
// model_close_calibrate(); model_quant() (test_quant.py:248-249): quantizer.scale / dic_scale / best_*
// lists.  p2v_forward walks the graph of VisionTransformer.forward_features/forward
// (models/vit_fquant.py:700-799) and enqueues 5 kernels per block on the caller's stream (LayerNorm+qkv, attention, proj+residual,
// LayerNorm+fc1+GELU, fc2+residual; 7 for models wider than the fused LayerNorm+GEMM kernel covers).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <memory>
#include <vector>

#include "p2vit_kernels.h"

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
// Graph capture (DESIGN "Graph capture of the forwards"): an entry point that copies from host memory of its own, synchronises, times with
// events or allocates cannot be recorded into a HIP graph - a capture records work, it does not run it.  Such an entry point asks here after
// its argument checks and before its first runtime call, enqueues nothing and leaves the capture valid.  A query that fails (no device, the
// null stream beside a capturing one) or reports an invalidated capture is NOT taken as capturing; the sticky error is cleared.
static bool stream_capturing(void* stream) {
  hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing((hipStream_t)stream, &status) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return status == hipStreamCaptureStatusActive;
}
static int refuse_capture(const char* who, const char* why, void* stream) {
  if (!stream_capturing(stream)) return P2V_OK;
  return fail(P2V_E_UNSUPPORTED, "%s: the stream is capturing a HIP graph and this call %s; make it outside the capture", who, why);
}
// a best-effort plan-time step (building tables a forward can do without) must not disturb p2v_last_error(): restored on the way out
struct KeepLastError {
  char keep[sizeof g_err];
  KeepLastError() { memcpy(keep, g_err, sizeof keep); }
  ~KeepLastError() { memcpy(g_err, keep, sizeof keep); }
};
static int launch_rc(int rc, const char* what) {
  if (rc == 0) return 0;
  if (rc == -2) return fail(P2V_E_UNSUPPORTED, "%s: s_qkv_sq * inv_s_attn must be a power of two", what);
  if (rc < 0) return fail(P2V_E_UNSUPPORTED, "%s: no kernel instantiated for this shape", what);
  return fail(P2V_E_LAUNCH, "%s: %s", what, hipGetErrorString((hipError_t)rc));
}
static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
static bool is_pot(float v) {
  int ex;
  return v > 0.f && frexpf(v, &ex) == 0.5f;
}

// ---- constant checks shared by the per-operator entry points and the plan setters: a plan that would make a kernel leave its
//      exact range is refused when it is built, not when (or, through p2v_forward, never) an operator is called
// exp_int = z * 2^(32-q) with z = r (r + b) + c: the kernels keep z exactly in fp32 and the table in int64
static int check_lis_consts(const char* who, int x0_int, int b_int, int c_int) {
  if (x0_int >= 0) return fail(P2V_E_ARG, "%s: x0_int must be negative", who);
  if (c_int <= 0 || c_int >= (1 << 24) || b_int < 0 || b_int >= (1 << 23) || x0_int < -(1 << 12))
    return fail(P2V_E_UNSUPPORTED, "%s: log-int-softmax constants out of range (x0 %d, b %d, c %d): softmax input scale below 2^-11?", who, x0_int,
                b_int, c_int);
  return P2V_OK;
}
static int check_requant_scale(const char* who, float inv_s_out) {
  if (!(is_pot(inv_s_out) && inv_s_out >= 0x1p-40f && inv_s_out <= 0x1p40f))
    return fail(P2V_E_UNSUPPORTED, "%s: REQUANT 1/scale %g must be a power of two (it is folded into the column scales)", who, inv_s_out);
  return P2V_OK;
}
static int check_gelu_tab(const char* who, const p2v_gelu_tab& t) {
  if (t.table && (t.cells <= 0 || t.cells > 4096)) return fail(P2V_E_ARG, "%s: GELU table with %d cells", who, t.cells);
  return P2V_OK;
}
// width of the log-int-softmax (the module's bit type, layers.py:372-375): uint4 or uint3
static int check_softmax_bits(const char* who, int bits) {
  if (bits != 3 && bits != 4) return fail(P2V_E_UNSUPPORTED, "%s: softmax_bits %d (the log-int-softmax runs at 3 or 4 bits)", who, bits);
  return P2V_OK;
}
// the probabilities enter the P.V product scaled by 2^-(127 - 2^bits) and av_mul carries the inverse (lis_prob_pair): the product stays a
// finite power of two up to 2^126, i.e. av_mul up to 2^15 at 4 bits and 2^7 at 3 bits
static float av_mul_max(int bits) { return bits == 3 ? 0x1p7f : 0x1p15f; }
static int check_attn(const char* who, const p2v_attn& at, int bits = 4) {
  if (const int rb = check_softmax_bits(who, bits)) return rb;
  const int rc = check_lis_consts(who, at.x0_int, at.b_int, at.c_int);
  if (rc != P2V_OK) return rc;
  // the kernel folds s_q1^2 / s_attn into qk_scale: exact only for a power of two (both are PoT scales in the reference)
  if (!is_pot(at.s_qkv_sq * at.inv_s_attn)) return fail(P2V_E_UNSUPPORTED, "%s: s_qkv_sq * inv_s_attn must be a power of two", who);
  if (!(at.qk_scale > 0.f) || !(at.av_mul > 0.f)) return fail(P2V_E_ARG, "%s: qk_scale and av_mul must be positive", who);
  // exact for a power of two in this range (s_q1 / qact2 scale of two PoT activation scales)
  if (!is_pot(at.av_mul) || at.av_mul > av_mul_max(bits) || at.av_mul < 0x1p-40f)
    return fail(P2V_E_UNSUPPORTED, "%s: av_mul %g must be a power of two in [2^-40, 2^%d] at softmax_bits %d", who, at.av_mul, bits == 3 ? 7 : 15, bits);
  return P2V_OK;
}

struct p2v_plan {
  p2v_model_desc d;
  int tokens, patches, k_patch, k_patch_pad, n_layers;
  std::vector<p2v_linear> lin[2];   // [bit index][layer]
  std::vector<char> lin_set[2];
  float inv_s_input;
  p2v_epilogue embed_epi;
  const int8_t* cls_codes;
  const int8_t* embed_cls_codes = nullptr;   // p2v_plan_set_embed_tap_cls: the class row of the qact_embed plane (FULL DDV stages), or null
  bool embed_set;
  std::vector<p2v_block> blocks;
  std::vector<char> block_set;
  p2v_ln final_ln;
  float head_inv_s, head_s;
  bool head_set;
  // LayerNorm constants folded at plan creation (p2v_ln.pre of the plan's copies of ln1 / ln2 / the final norm): the arrays live in one device
  // buffer per block (+ one for the final norm), owned by the plan
  std::vector<float*> ln_pre_buf;
  float* final_pre_buf = nullptr;
  std::vector<char> block_folded;
  // tables of the pre-folded RESID epilogue (p2v_resid_prefold): [block][proj = 0 / fc2 = 1][bit index]; null = the generic epilogue.  One device
  // buffer per block, owned by the plan
  std::vector<const float*> resid_tab;
  std::vector<float*> resid_buf;
  int device = -1;                  // the device that owns the folded constants (= the device of the caller's arrays)
  // Config(ptf=False) / Config(lis=False): float LayerNorm and table softmax (p2v_plan_set_float_ops / _float_block / _float_head)
  bool float_norm = false, float_softmax = false, fhead_set = false;
  std::vector<p2v_float_block> fblocks;
  std::vector<char> fblock_set;
  p2v_float_ln final_fln = {};
  std::vector<char> softmax_bits;   // [block] width of the block's log-int-softmax (p2v_plan_set_softmax_bits): 4 unless set
  // p2v_plan_prepare_grams: of every per-channel stage scale vector its exponent bytes (one device buffer, owned by the plan) and its unit
  struct GramScale { const float* scale; const uint8_t* shift; double unit; };
  std::vector<GramScale> gram_scales;
  uint8_t* gram_shift_buf = nullptr;
  bool grams_ready = false;
  ~p2v_plan() {
    int prev = -1;
    const bool sw = device >= 0 && hipGetDevice(&prev) == hipSuccess && prev != device && hipSetDevice(device) == hipSuccess;
    for (float* b : ln_pre_buf)
      if (b) (void)hipFree(b);
    for (float* b : resid_buf)
      if (b) (void)hipFree(b);
    if (final_pre_buf) (void)hipFree(final_pre_buf);
    if (gram_shift_buf) (void)hipFree(gram_shift_buf);
    if (sw) (void)hipSetDevice(prev);
  }
};

static void build_resid_tables(p2v_plan* plan, int block);
static int bit_index(int bits) { return bits == 4 ? 0 : (bits == 8 ? 1 : -1); }
// LayerNorm i of a block's six: ln1[0 .. 1], then ln2[0 .. 1][0 .. 1]
template <class Block>
static auto& block_ln(Block& b, int i) { return i < 2 ? b.ln1[i] : b.ln2[(i - 2) >> 1][(i - 2) & 1]; }
static bool ln_constants_present(const p2v_ln& l, bool with_mask = true) {
  return (l.mask || !with_mask) && l.gamma && l.beta && l.inv_out && l.post_mul;
}

extern "C" {

extern int g_ln_generic;
extern int g_ln_rows;
extern int g_attn_waves;
extern int g_ln_gemm;
extern int g_ln_gemm_ver;
extern int g_ln_gemm_lean;
extern int g_gemm_tile;
extern int g_resid_pre;
extern int g_attn_stream;
extern int g_attn_packed;
extern int g_ln_pre;
extern int g_gemm_rows;
int g_cls_rows = 1;       // 0: the last block of p2v_forward computes every row, as the other blocks do (A/B and parity runs)

// The tuning / A-B switches: the name p2v_set_tuning knows, the environment variable read once per process (first plan or first version
// query), and the accepted values lo, lo + step ... hi.  None of them changes results (ln_generic forces the generic LayerNorm chain:
// bit-identical to the fast one, both are tested).  An on / off switch (0 .. 1) may take ANY integer as "not zero", separately for the two
// ways in: all of them do through p2v_set_tuning except cls_rows, all of them do from the environment except ln_generic (whose only
// effective setting there is 1: the variable starts at 0).
enum { ANY_ENV = 1, ANY_API = 2 };
static const struct Switch {
  const char *name, *env;
  int* var;
  int lo, hi, step, any;
  bool takes(int v, int how) const { return (any & how) || (v >= lo && v <= hi && (v - lo) % step == 0); }
  void set(int v) const { *var = (hi == 1 && lo == 0) ? v != 0 : v; }
} kSwitches[] = {
    {"attn_waves", "P2V_ATTN_WAVES", &g_attn_waves, 4, 8, 1, 0},
    {"ln_gemm", "P2V_LN_GEMM", &g_ln_gemm, 0, 1, 1, ANY_ENV | ANY_API},
    {"ln_gemm_version", "P2V_LN_GEMM_V", &g_ln_gemm_ver, 1, 3, 1, 0},
    {"gemm_tile", "P2V_GEMM_TILE", &g_gemm_tile, 0, 256, 128, 0},
    {"attn_stream", "P2V_ATTN_STREAM", &g_attn_stream, 0, 1, 1, ANY_ENV | ANY_API},
    {"attn_packed", "P2V_ATTN_PACKED", &g_attn_packed, 0, 1, 1, 0},
    {"ln_pre", "P2V_LN_PRE", &g_ln_pre, 0, 1, 1, ANY_ENV | ANY_API},
    {"resid_pre", "P2V_RESID_PRE", &g_resid_pre, 0, 1, 1, ANY_ENV | ANY_API},
    {"gemm_rows", "P2V_GEMM_ROWS", &g_gemm_rows, 0, 2, 1, 0},
    {"cls_rows", "P2V_CLS_ROWS", &g_cls_rows, 0, 1, 1, ANY_ENV},
    {"ln_rows", "P2V_LN_ROWS", &g_ln_rows, 1, 64, 1, 0},
    {"ln_generic", "P2V_LN_GENERIC", &g_ln_generic, 0, 1, 1, ANY_API},
    {"ln_gemm_lean", "P2V_LN_GEMM_LEAN", &g_ln_gemm_lean, 0, 1, 1, ANY_ENV | ANY_API},
};

static void read_env_once() {
  static bool done = false;
  if (done) return;
  done = true;
  for (const Switch& s : kSwitches) {
    const char* e = getenv(s.env);
    if (e && s.takes(atoi(e), ANY_ENV)) s.set(atoi(e));          // a value out of range is ignored
  }
}
int p2v_abi_version(void) { read_env_once(); return P2V_ABI_VERSION; }

int p2v_resident_tokens(int head_dim) { return p2v_resident_tokens_of(head_dim); }
int p2v_max_tokens(int head_dim) { return p2v_resident_tokens_of(head_dim) ? P2V_MAX_TOKENS_STREAMED : 0; }
int p2v_packed_tokens(int head_dim) { return head_dim == 64 ? P2V_MAX_TOKENS_PACKED : 0; }
int p2v_attention_kernel(int head_dim, int tokens, int tapped) {
  read_env_once();
  return p2v_attention_kernel_of(head_dim, tokens, tapped);
}

int p2v_set_tuning(const char* name, int value) {
  if (!name) return fail(P2V_E_ARG, "p2v_set_tuning: null name");
  read_env_once();                      // an explicit setting wins over the environment
  for (const Switch& s : kSwitches)
    if (!strcmp(name, s.name) && s.takes(value, ANY_API)) {
      s.set(value);
      return P2V_OK;
    }
  return fail(P2V_E_ARG, "p2v_set_tuning: unknown switch or value out of range: %s = %d", name, value);
}
const char* p2v_last_error(void) { return g_err; }

int p2v_plan_create(const p2v_model_desc* desc, p2v_plan** out) {
  if (!desc || !out) return fail(P2V_E_ARG, "p2v_plan_create: null argument");
  read_env_once();
  if (desc->abi_version != P2V_ABI_VERSION) return fail(P2V_E_ARG, "ABI version %d != %d", desc->abi_version, P2V_ABI_VERSION);
  const p2v_model_desc& d = *desc;
  if (d.img_size <= 0 || d.patch_size <= 0 || d.img_size % d.patch_size) return fail(P2V_E_SHAPE, "img_size %% patch_size != 0");
  if (d.patch_size % 4) return fail(P2V_E_UNSUPPORTED, "patch_size must be a multiple of 4");
  if (d.embed_dim % d.num_heads) return fail(P2V_E_SHAPE, "embed_dim %% num_heads != 0");
  const int hd = d.embed_dim / d.num_heads;
  if (hd != 32 && hd != 48 && hd != 64 && hd != 80 && hd != 96 && hd != 128)
    return fail(P2V_E_UNSUPPORTED, "head_dim %d (32, 48, 64, 80, 96 and 128 are instantiated)", hd);
  // rows are read in 16-byte pieces and stored 16 channels at a time; widths that are not multiples of the 64-deep k-tile run through zero
  // weight columns (the tile's last pieces then belong to the next row of the workspace buffer: multiplied by zero)
  if (d.embed_dim % 16 || d.mlp_hidden % 16) return fail(P2V_E_UNSUPPORTED, "embed_dim and mlp_hidden must be multiples of 16");
  {   // the resident attention kernel keeps a query block's scores in registers and K / V^T of an image's head in LDS (p2v_resident_tokens); the
      // streaming kernel takes over beyond, up to 4096 tokens per image
    const int tokens = (d.img_size / d.patch_size) * (d.img_size / d.patch_size) + 1;
    if (tokens > P2V_MAX_TOKENS_STREAMED)
      return fail(P2V_E_UNSUPPORTED, "%d tokens per image: the attention kernels cover up to %d", tokens, P2V_MAX_TOKENS_STREAMED);
  }
  if (d.embed_dim > 2048) return fail(P2V_E_UNSUPPORTED, "embed_dim %d: the LayerNorm kernel covers up to 2048 channels", d.embed_dim);
  p2v_plan* p = new p2v_plan();
  p->d = d;
  p->patches = (d.img_size / d.patch_size) * (d.img_size / d.patch_size);
  p->tokens = p->patches + 1;
  p->k_patch = d.in_chans * d.patch_size * d.patch_size;
  p->k_patch_pad = round_up(p->k_patch, GBK_PAD);
  p->n_layers = 4 * d.depth + 2;
  for (int b = 0; b < 2; ++b) {
    p->lin[b].assign(p->n_layers, p2v_linear{nullptr, nullptr, nullptr, nullptr, 0});
    p->lin_set[b].assign(p->n_layers, 0);
  }
  p->blocks.resize(d.depth);
  p->block_set.assign(d.depth, 0);
  p->ln_pre_buf.assign(d.depth, nullptr);
  p->block_folded.assign(d.depth, 0);
  p->resid_tab.assign((size_t)d.depth * 4, nullptr);
  p->resid_buf.assign(d.depth, nullptr);
  p->embed_set = p->head_set = false;
  p->cls_codes = nullptr;
  p->fblocks.resize(d.depth);
  p->fblock_set.assign(d.depth, 0);
  p->softmax_bits.assign(d.depth, 4);
  *out = p;
  return P2V_OK;
}

void p2v_plan_destroy(p2v_plan* plan) { delete plan; }

int p2v_plan_set_linear(p2v_plan* plan, int layer, int bits, const p2v_linear* lin) {
  if (!plan || !lin) return fail(P2V_E_ARG, "p2v_plan_set_linear: null argument");
  const int bi = bit_index(bits);
  if (bi < 0) return fail(P2V_E_BITS, "bits %d not in {4, 8}", bits);
  if (layer < 0 || layer >= plan->n_layers) return fail(P2V_E_ARG, "layer %d out of range [0,%d)", layer, plan->n_layers);
  if (!lin->w_codes || !lin->colscale || !lin->bias) return fail(P2V_E_ARG, "p2v_plan_set_linear: null device pointer");
  if (lin->packed4 && bits != 4) return fail(P2V_E_BITS, "packed4 weights for a %d-bit layer", bits);
  plan->lin[bi][layer] = *lin;
  plan->lin_set[bi][layer] = 1;
  if (layer >= 1 && layer < plan->n_layers - 1 && ((layer - 1) & 1)) {         // proj / fc2 of block (layer - 1) / 4: their RESID tables depend on these constants
    const int block = (layer - 1) / 4;
    if (plan->block_set[block]) build_resid_tables(plan, block);
  }
  return P2V_OK;
}

int p2v_plan_set_embed(p2v_plan* plan, float inv_s_input, const p2v_epilogue* e, const int8_t* cls_row_codes) {
  if (!plan || !e || !cls_row_codes) return fail(P2V_E_ARG, "p2v_plan_set_embed: null argument");
  plan->inv_s_input = inv_s_input;
  plan->embed_epi = *e;
  plan->embed_epi.patches = plan->patches;
  plan->cls_codes = cls_row_codes;
  plan->embed_set = true;
  return P2V_OK;
}

int p2v_plan_set_embed_tap_cls(p2v_plan* plan, const int8_t* cls_embed_codes) {
  if (!plan || !cls_embed_codes) return fail(P2V_E_ARG, "p2v_plan_set_embed_tap_cls: null argument");
  plan->embed_cls_codes = cls_embed_codes;
  return P2V_OK;
}

// Make the device that owns `ptr` current for the lifetime of the object (plan-time folds run hipMalloc / copies / small kernels next to the
// caller's arrays, whatever device the process has selected); ok() is false when the owner cannot be determined.
struct OwnerDevice {
  int prev = -1, own = -1;
  explicit OwnerDevice(const void* ptr) {
    hipPointerAttribute_t pa;
    if (hipGetDevice(&prev) != hipSuccess || hipPointerGetAttributes(&pa, ptr) != hipSuccess) {
      (void)hipGetLastError();
      return;
    }
    if (pa.type != hipMemoryTypeDevice && pa.type != hipMemoryTypeManaged) return;      // host memory (registered or not): not ours to launch on
    own = pa.device;
    if (own != prev && hipSetDevice(own) != hipSuccess) own = -1;
  }
  ~OwnerDevice() { if (own >= 0 && own != prev) (void)hipSetDevice(prev); }
  bool ok() const { return own >= 0; }
};

static size_t resid_tab_floats(int N) { return (size_t)((N + 127) / 128) * 6 * 128; }

// build one table on the current device; *usable = 0 when the pre-folded form is not provably the reference's for these constants
static int resid_prefold_impl(const p2v_linear& lin, const p2v_epilogue& ep, int N, float* tab, int* usable, hipStream_t st) {
  *usable = 0;
  unsigned* flags = nullptr;
  hipError_t e = hipMalloc(&flags, 2 * sizeof(unsigned));
  const unsigned init[2] = {1u, 0u};
  unsigned got[2] = {0u, 0u};
  if (e == hipSuccess) e = hipMemcpyAsync(flags, init, sizeof init, hipMemcpyHostToDevice, st);
  int rc = 0;
  if (e == hipSuccess) rc = p2v_launch_resid_prefold(lin, ep, N, tab, flags, st);
  if (e == hipSuccess && rc == 0) e = hipMemcpyAsync(got, flags, sizeof got, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && rc == 0) e = hipStreamSynchronize(st);
  if (flags) (void)hipFree(flags);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(P2V_E_LAUNCH, "resid_prefold: %s", hipGetErrorString(e));
  }
  if (rc) return launch_rc(rc, "resid_prefold");
  *usable = got[0] ? 1 : 0;
  return P2V_OK;
}

// (Re)build the RESID tables of a block for every bit width whose weights are set; called from both setters, whichever comes last.
// Best effort: unusable tables simply leave the generic RESID epilogue in place.
static void build_resid_tables(p2v_plan* plan, int block) {
  KeepLastError keep;
  for (int j = 0; j < 4; ++j) plan->resid_tab[(size_t)block * 4 + j] = nullptr;
  if (!plan->block_set[block]) return;
  const p2v_block& blk = plan->blocks[block];
  OwnerDevice dev(blk.proj_epi.s_mid);
  if (!dev.ok() || (plan->device >= 0 && plan->device != dev.own)) return;
  const int D = plan->d.embed_dim;
  const size_t per = resid_tab_floats(D);
  if (hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); return; }      // the caller's uploads may still be in flight
  float* buf = plan->resid_buf[block];
  if (!buf && hipMalloc(&buf, 4 * per * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return; }
  plan->resid_buf[block] = buf;
  plan->device = dev.own;
  for (int which = 0; which < 2; ++which)
    for (int bi = 0; bi < 2; ++bi) {
      const int layer = 1 + 4 * block + (which ? 3 : 1);
      if (!plan->lin_set[bi][layer]) continue;
      int usable = 0;
      float* tab = buf + (size_t)(which * 2 + bi) * per;
      if (resid_prefold_impl(plan->lin[bi][layer], which ? blk.fc2_epi : blk.proj_epi, D, tab, &usable, nullptr) == P2V_OK && usable)
        plan->resid_tab[(size_t)block * 4 + which * 2 + bi] = tab;
    }
}

// The fold of ln_prepare (p2vit_ln.hip), once per LayerNorm instead of once per workgroup: the same fp32 products and the same tests on the
// host (this file is compiled without contraction too); `dev` receives gamma / out_scale and beta / out_scale, each padded with zeros to
// Cp = round_up(C, 256) channels.  The current device must be the one that owns the arrays.
static hipError_t fold_one_ln(const p2v_ln& l, int C, float* dev, p2v_ln_pre* out) {
  const int Cp = round_up(C, 256);                             // (a row group of 64 lanes covers 256 channels per chunk)
  std::vector<float> g(C), b(C), io(C), pm(C), host((size_t)2 * Cp, 0.f);
  hipError_t e = hipMemcpy(g.data(), l.gamma, C * sizeof(float), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(b.data(), l.beta, C * sizeof(float), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(io.data(), l.inv_out, C * sizeof(float), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(pm.data(), l.post_mul, C * sizeof(float), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return e;
  float* go = host.data();
  float* bo = go + Cp;
  int pot = 1, pm1 = 1;
  float gmin = 3.0e38f, gmax = 0.f, bmax = 0.f;
  for (int c = 0; c < C; ++c) {
    unsigned ib;
    memcpy(&ib, &io[c], 4);
    const int p2 = (int)((ib & 0x807FFFFFu) == 0u) & (int)((ib >> 23) - 32u <= 190u);    // +2^e, far from under/overflow
    go[c] = g[c] * io[c];
    bo[c] = b[c] * io[c];
    const float ga = fabsf(go[c]), ba = fabsf(bo[c]);
    const int gok = (int)(g[c] == 0.f) | ((int)(ga >= 1.0e-30f) & (int)(ga <= 1.0e30f));
    const int bok = (int)(b[c] == 0.f) | ((int)(ba >= 1.0e-30f) & (int)(ba <= 1.0e30f));
    pot &= p2 & gok & bok;
    pm1 &= (int)(pm[c] == 1.f);
    gmin = fminf(gmin, ga);
    gmax = fmaxf(gmax, ga);
    bmax = fmaxf(bmax, ba);
  }
  e = hipMemcpy(dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) *out = p2v_ln_pre{dev, dev + Cp, gmin, gmax, bmax, pot, pm1};
  return e;
}
static const p2v_ln_pre kNoPre = {nullptr, nullptr, 0.f, 0.f, 0.f, 0, 0};

// The plan's six LayerNorms of a block, folded on the device that OWNS the caller's arrays, whatever the process's current device is (a
// plan built for cuda:1 while cuda:0 is current).  Returns false, with the reason in p2v_last_error(), when the constants could not be
// folded: the block's kernels then fold per workgroup, with the same results.
static bool fold_ln_constants(p2v_plan* plan, int block) {
  const int C = plan->d.embed_dim, Cp = round_up(C, 256);
  p2v_block& blk = plan->blocks[block];
  // stale state first: a second p2v_plan_set_block on this block must never leave the constants of the previous arrays behind
  for (int i = 0; i < 6; ++i) block_ln(blk, i).pre = kNoPre;
  OwnerDevice own(blk.ln1[0].gamma);
  if (!own.ok()) {
    fail(P2V_OK, "p2v_plan_set_block: LayerNorm constants of block %d not folded at plan time (cannot locate the device of gamma)", block);
    return false;
  }
  if (plan->device >= 0 && plan->device != own.own) {
    fail(P2V_OK, "p2v_plan_set_block: block %d lives on device %d, earlier blocks on device %d: not folded at plan time", block, own.own, plan->device);
    return false;
  }
  hipError_t e = hipDeviceSynchronize();                        // the caller's uploads may still be in flight on another stream
  float* dev = plan->ln_pre_buf[block];
  if (e == hipSuccess && !dev) e = hipMalloc(&dev, (size_t)12 * Cp * sizeof(float));
  p2v_ln_pre pre[6];
  if (e == hipSuccess) {
    plan->ln_pre_buf[block] = dev;
    plan->device = own.own;
    for (int i = 0; i < 6 && e == hipSuccess; ++i) e = fold_one_ln(block_ln(blk, i), C, dev + (size_t)(2 * i) * Cp, &pre[i]);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();                                    // do not leave the error for an unrelated CHECK_LAUNCH
    fail(P2V_OK, "p2v_plan_set_block: LayerNorm constants of block %d not folded at plan time (%s)", block, hipGetErrorString(e));
    return false;
  }
  for (int i = 0; i < 6; ++i) block_ln(blk, i).pre = pre[i];
  return true;
}

int p2v_plan_set_block(p2v_plan* plan, int block, const p2v_block* blk) {
  if (!plan || !blk) return fail(P2V_E_ARG, "p2v_plan_set_block: null argument");
  if (block < 0 || block >= plan->d.depth) return fail(P2V_E_ARG, "block %d out of range", block);
  // p2v_forward launches the kernels directly: everything the per-operator entry points check is checked here, once
  int rc = check_attn("p2v_plan_set_block: attn", blk->attn, plan->softmax_bits[block]);
  if (rc == P2V_OK) rc = check_gelu_tab("p2v_plan_set_block: gelu_fc1", blk->gelu_fc1);
  for (int b = 0; b < 2 && rc == P2V_OK; ++b) rc = check_requant_scale("p2v_plan_set_block: inv_s_qkv", blk->inv_s_qkv[b]);
  if (rc == P2V_OK && !(is_pot(blk->inv_s_fc1) && blk->inv_s_fc1 >= 0x1p-40f && blk->inv_s_fc1 <= 0x1p40f))
    rc = fail(P2V_E_UNSUPPORTED, "p2v_plan_set_block: 1/scale of mlp.qact1 %g must be a power of two", blk->inv_s_fc1);
  if (rc == P2V_OK && (!blk->proj_epi.s_mid || !blk->proj_epi.s_res || !blk->proj_epi.s_next || !blk->fc2_epi.s_mid || !blk->fc2_epi.s_res ||
                       !blk->fc2_epi.s_next))
    rc = fail(P2V_E_ARG, "p2v_plan_set_block: RESID epilogues need s_mid/s_res/s_next");
  for (int i = 0; i < 6 && rc == P2V_OK; ++i)
    if (!ln_constants_present(block_ln(*blk, i))) rc = fail(P2V_E_ARG, "p2v_plan_set_block: LayerNorm constants missing");
  if (rc != P2V_OK) return rc;
  plan->blocks[block] = *blk;
  plan->block_set[block] = 1;
  // without the fold the kernels fold per workgroup, as for the per-operator calls: same results, so the call still succeeds; the reason
  // is left in p2v_last_error() and p2v_plan_block_prefolded() tells
  g_err[0] = 0;
  plan->block_folded[block] = fold_ln_constants(plan, block) ? 1 : 0;
  build_resid_tables(plan, block);
  return P2V_OK;
}

int p2v_plan_block_prefolded(const p2v_plan* plan, int block) {
  if (!plan || block < 0 || block >= plan->d.depth) return fail(P2V_E_ARG, "p2v_plan_block_prefolded: bad argument");
  return plan->block_folded[block] ? 1 : 0;
}

int p2v_plan_resid_prefolded(const p2v_plan* plan, int block) {
  if (!plan || block < 0 || block >= plan->d.depth) return fail(P2V_E_ARG, "p2v_plan_resid_prefolded: bad argument");
  int m = 0;
  for (int j = 0; j < 4; ++j) m |= plan->resid_tab[(size_t)block * 4 + j] ? 1 << j : 0;
  return m;
}

int p2v_plan_set_head(p2v_plan* plan, const p2v_ln* final_ln, float inv_s_out, float s_out) {
  if (!plan || !final_ln) return fail(P2V_E_ARG, "p2v_plan_set_head: null argument");
  if (!ln_constants_present(*final_ln))
    return fail(P2V_E_ARG, "p2v_plan_set_head: LayerNorm constants missing");
  if (!(inv_s_out > 0.f) || !(s_out > 0.f)) return fail(P2V_E_ARG, "p2v_plan_set_head: act_out scale must be positive");
  plan->final_ln = *final_ln;
  plan->final_ln.pre = kNoPre;
  {   // the final norm's constants, folded like a block's (best effort: the per-workgroup fold gives the same codes)
    OwnerDevice own(final_ln->gamma);
    const int C = plan->d.embed_dim;
    if (own.ok() && (plan->device < 0 || plan->device == own.own) && hipDeviceSynchronize() == hipSuccess) {
      if (!plan->final_pre_buf && hipMalloc(&plan->final_pre_buf, (size_t)2 * round_up(C, 256) * sizeof(float)) != hipSuccess) plan->final_pre_buf = nullptr;
      p2v_ln_pre pre;
      if (plan->final_pre_buf && fold_one_ln(*final_ln, C, plan->final_pre_buf, &pre) == hipSuccess) {
        plan->final_ln.pre = pre;
        plan->device = own.own;
      }
    }
    (void)hipGetLastError();
  }
  plan->head_inv_s = inv_s_out;
  plan->head_s = s_out;
  plan->head_set = true;
  return P2V_OK;
}

// workspace: [patches | x | ln | qkv | att | hid | cls], each 256-byte aligned
struct WsLayout {
  size_t patches, x, ln, qkv, att, hid, cls, total;
};
static WsLayout ws_layout(const p2v_plan* p, int batch) {
  auto al = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t M = (size_t)batch * p->tokens, D = p->d.embed_dim;
  WsLayout w;
  size_t off = 0;
  w.patches = off; off += al((size_t)batch * p->patches * p->k_patch_pad);
  w.x = off;       off += al(M * D);
  w.ln = off;      off += al(M * D);
  w.qkv = off;     off += al(M * 3 * D);
  w.att = off;     off += al(M * D);
  w.hid = off;     off += al(M * (size_t)p->d.mlp_hidden);
  w.cls = off;     off += al((size_t)batch * D);
  w.total = off + 256;     // a k-tile of the last row of the last buffer may reach up to 48 bytes past the row (widths not a multiple of 64)
  return w;
}

size_t p2v_workspace_bytes(const p2v_plan* plan, int batch) {
  if (!plan || batch <= 0) return 0;
  return ws_layout(plan, batch).total;
}

long long p2v_workspace_view(const p2v_plan* plan, int batch, const char* name) {
  if (!plan || !name || batch <= 0) return -1;
  const WsLayout w = ws_layout(plan, batch);
  const struct { const char* name; size_t off; } views[] = {{"patches", w.patches}, {"x", w.x}, {"ln", w.ln}, {"qkv", w.qkv}, {"att", w.att}, {"hid", w.hid}, {"cls", w.cls}};
  for (const auto& v : views)
    if (!strcmp(name, v.name)) return (long long)v.off;
  return -1;
}

}  // extern "C"

// ---- the whole-model forward ------------------------------------------------------------------------------------------------------------
// The one place a GemmArgs is filled.  W: the layer's weights in the layout the kernel reads (lin.w_codes, or lin.w_frag for the fused
// LayerNorm+GEMM kernels); K in whole k-tiles
static GemmArgs gemm_args(const int8_t* A, int lda, int M, const int8_t* W, int K, int N, const p2v_linear& lin, const p2v_epilogue& ep,
                          void* out, int ldo, int8_t* out_codes) {
  GemmArgs g;
  g.A = A; g.lda = lda; g.M = M; g.W = W; g.K = K; g.N = N; g.w4 = lin.packed4 ? 1 : 0;
  g.colscale = lin.colscale; g.bias = lin.bias; g.ep = ep; g.out = out; g.ldo = ldo; g.out_codes = out_codes; g.out_codes2 = nullptr; g.tiles_n = 0;
#ifdef P2V_DIAG
  g.stamps = nullptr;
#endif
  return g;
}

// few_rows: a layer GEMM over the few class-token rows - the row kernel unless the switches name the tiled one (gemm_rows = 2, or an explicit gemm_tile)
static int run_gemm(int epi, const int8_t* A, int lda, int M, int K, int N, const p2v_linear& lin, const p2v_epilogue& ep, void* out,
                    int ldo, int8_t* out_codes, hipStream_t st, bool few_rows = false) {
  const GemmArgs g = gemm_args(A, lda, M, lin.w_codes, K, N, lin, ep, out, ldo, out_codes);
  if (few_rows && g_gemm_rows != 2 && g_gemm_tile == 0 && !(epi == P2V_EPI_RESID && out_codes)) return launch_rc(p2v_launch_gemm_rows(epi, g, st), "gemm_rows");
  const int rc = p2v_launch_gemm(epi, g, st);
  if (rc == -4) {      // the tiled kernel's 32-bit lane offsets: name the bound that is passed, as p2v_gemm_resid_tap does for M * ldo
    const long long a_bytes = (long long)M * lda + K, w_bytes = (long long)((N + 127) / 128) * 128 * K;
    if (a_bytes >= (1LL << 32))
      return fail(P2V_E_UNSUPPORTED, "gemm_i8: M * lda + K = %lld must stay below 2^32 = 4294967296, the 32-bit lane offsets of the tiled kernel", a_bytes);
    return fail(P2V_E_UNSUPPORTED, "gemm_i8: round_up(N, 128) * K = %lld must stay below 2^32 = 4294967296, the 32-bit lane offsets of the tiled kernel", w_bytes);
  }
  return launch_rc(rc, "gemm_i8");
}

// QIntLayerNorm -> /cs -> qact0 -> QLinear -> (GELU) -> QAct in one launch (k_ln_gemm); a.out may be null
static int run_ln_gemm(int epi, const LnArgs& a, const p2v_linear& lin, const p2v_epilogue& ep, int N, int8_t* out, hipStream_t st) {
  if (!lin.w_frag) return fail(P2V_E_UNSUPPORTED, "ln_gemm: the layer has no fragment-order weights (p2v_linear.w_frag)");
  const int rc = p2v_launch_ln_gemm(epi, a, gemm_args(nullptr, a.C, (int)a.rows, lin.w_frag, round_up(a.C, GBK_PAD), N, lin, ep, out, N, nullptr), st);
  if (rc == -3) return fail(P2V_E_UNSUPPORTED, "ln_gemm: shape C=%d N=%d is not fused", a.C, N);
  return launch_rc(rc, "ln_gemm");
}

struct Prof {
  std::vector<hipEvent_t> ev;   // a pool created BEFORE the enqueue loop (an event created between two launches paces the host, and the
                                // interval it opens then measures the host, not the kernel); ev[i] is recorded before launch i, one more after the last
  std::vector<int> kind;        // P2V_K_* of launch i
  int used = 0;
  hipStream_t st = nullptr;     // the stream of the pass: p2v_forward_profile_end asks it whether it is capturing by then
  bool make_pool(int n) {
    ev.resize(n);
    kind.reserve(n);
    for (int i = 0; i < n; ++i)
      if (hipEventCreate(&ev[i]) != hipSuccess) { ev.resize(i); return false; }
    return true;
  }
  ~Prof() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};
static int prof_pool_size(const p2v_plan* p) { return p ? 7 * p->d.depth + 10 : 0; }

// p2v_forward_ddv: the batch is n clean images followed by their n perturbed twins; after the launch that completes a stage its rows
// [0, n * T) are reduced against rows [n * T, 2n * T) (p2vit_ddv.hip), stage k into sums[k][n][3]
struct DdvCtx {
  int n;
  unsigned long long* partials;   // `slots` workgroup partials of 3 values, reused by every stage (one stream)
  long long slots;
  double* sums;
  float* tap;                     // the one fp32 tap buffer of with_linear, or null
  int stage;
  float* scratch = nullptr;       // P2V_DDV_STAGES_FULL: the same buffer, for the fp32 LayerNorm values (set whatever with_linear says); null = the engine stages
  int8_t* attn = nullptr;         // P2V_DDV_STAGES_ATTN: the two planes of one block's attention taps (p2v_ddv_attn_scratch_bytes); null = no such stages
  struct StatsCtx* stats = nullptr;   // p2v_forward_stats: the stage sites reduce all n samples into records instead of pairs into cosines
  struct GramsCtx* grams = nullptr;   // p2v_forward_grams: the stage sites take the n x n Gram of all n samples
};
// p2v_forward_stats: stage k's record lies at the running offset in the arena; a layout pass (no launches) lists the records instead
struct StatsStage { size_t off; int cols, kind; const float* scale; };
struct StatsCtx {
  char* arena;
  size_t bytes, off;
  std::vector<StatsStage>* layout;    // non-null: the layout pass
};
static int stats_check(const p2v_stat_layer& a, const void* rec, bool aligned, const char* what, int l);
static int stats_reduce(DdvCtx* c, const void* base, int rows, int cols, int dtype, const float* scale, hipStream_t st, long long sample_stride,
                        long long row_stride) {
  StatsCtx* s = c->stats;
  const int kind = dtype == P2V_COS_F32 ? P2V_STAT_F32 : dtype == P2V_COS_LOG2K ? P2V_STAT_U8 : P2V_STAT_I8;      // (I8_DEQ: the codes, its scales in the layout)
  const size_t off = s->off;
  s->off += p2v_stats_bytes(cols);
  ++c->stage;
  if (s->layout) {
    s->layout->push_back(StatsStage{off, cols, kind, scale});
    return P2V_OK;
  }
  if (s->off > s->bytes) return fail(P2V_E_WORKSPACE, "p2v_forward_stats: the records need more than %zu bytes", s->bytes);
  const p2v_stat_layer l{base, sample_stride, row_stride, c->n, rows, cols, kind};
  const int rc = stats_check(l, s->arena + off, false, "p2v_forward_stats", c->stage - 1);
  return rc != P2V_OK ? rc : launch_rc(p2v_launch_stats(p2v_stats_desc(l, s->arena + off), st), "stage_stats");
}
// p2v_forward_grams: stage k's Gram goes to grams[k][n][n], its unit to units[k]; a layout pass (no launches) lists the stages instead
struct GramStage { int rows, cols, kind; const float* scale; };
struct GramsCtx {
  const p2v_plan* plan;
  double *grams, *units;
  void* ws;                           // the partials of one stage, reused by every stage (one stream)
  size_t ws_bytes;
  std::vector<GramStage>* layout;     // non-null: the layout pass
  std::vector<double> host_units;     // uploaded once behind the last stage
};
static int gram_check(const p2v_gram_layer& a, int n, bool aligned, const char* what, int l);
static size_t gram_ws_bytes(const p2v_gram_layer& a, int n);
static int gram_launch(const p2v_gram_layer& a, int n, double* G, void* ws, hipStream_t st);
static int grams_reduce(DdvCtx* c, const void* base, int rows, int cols, int dtype, const float* scale, hipStream_t st, long long sample_stride,
                        long long row_stride) {
  GramsCtx* g = c->grams;
  const int k = c->stage++;
  const int kind = dtype == P2V_COS_F32 ? P2V_GRAM_F32 : P2V_GRAM_I8;
  if (dtype == P2V_COS_LOG2K) return fail(P2V_E_UNSUPPORTED, "p2v_forward_grams: the exponent planes of the attention stages are no byte codes");
  if (g->layout) {
    g->layout->push_back(GramStage{rows, cols, kind, scale});
    return P2V_OK;
  }
  const uint8_t* shift = nullptr;
  double unit = kind == P2V_GRAM_F32 ? 1.0 : 0.0;
  if (scale) {
    const p2v_plan::GramScale* hit = nullptr;
    for (const p2v_plan::GramScale& s : g->plan->gram_scales)
      if (s.scale == scale) { hit = &s; break; }
    if (!hit) return fail(P2V_E_STATE, "p2v_forward_grams: stage %d has per-channel scales p2v_plan_prepare_grams has not seen", k);
    shift = hit->shift;
    unit = hit->unit;
  }
  const p2v_gram_layer l{base, shift, sample_stride, row_stride, rows, cols, kind};
  int rc = gram_check(l, c->n, false, "p2v_forward_grams", k);
  if (rc != P2V_OK) return rc;
  if (gram_ws_bytes(l, c->n) > g->ws_bytes)
    return fail(P2V_E_WORKSPACE, "p2v_forward_grams: stage %d needs %zu bytes of partials, the workspace holds %zu", k, gram_ws_bytes(l, c->n), g->ws_bytes);
  g->host_units.push_back(unit);
  return launch_rc(gram_launch(l, c->n, g->grams + (size_t)k * c->n * c->n, g->ws, st), "stage_gram");
}
// sample_stride (elements): 0 = the samples are dense, rows * cols apart; else e.g. the patch rows of a [T][cols] token layout
// row_stride (elements): 0 = dense rows; else the pitch of the attention planes
static int ddv_reduce(DdvCtx* c, const void* base, int rows, int cols, int dtype, const float* scale, hipStream_t st, long long sample_stride = 0,
                      long long row_stride = 0) {
  const size_t esz = dtype == P2V_COS_F32 ? 4 : 1;
  if (!row_stride) row_stride = cols;
  if (!sample_stride) sample_stride = (long long)rows * row_stride;
  if (c->stats) return stats_reduce(c, base, rows, cols, dtype, scale, st, sample_stride, row_stride);
  if (c->grams) return grams_reduce(c, base, rows, cols, dtype, scale, st, sample_stride, row_stride);
  const p2v_cos_layer l{base, reinterpret_cast<const char*>(base) + (size_t)c->n * sample_stride * esz, scale, sample_stride, row_stride, rows, cols, dtype};
  const CosDesc d = p2v_cos_desc(l, c->n, 0);        // (logits / head rows of a class count that is no multiple of 4: d.vec = 0, scalar loads)
  if ((long long)c->n * d.nsplit > c->slots)
    return fail(P2V_E_WORKSPACE, "p2v_forward_ddv: a stage of %d x %d needs %lld partials, the workspace holds %lld", rows, cols,
                (long long)c->n * d.nsplit, c->slots);
  const int rc = launch_rc(p2v_launch_pair_cosine_one(d, c->n, c->partials, c->sums + (size_t)c->stage * c->n * 3, st), "pair_cosine");
  ++c->stage;
  return rc;
}

// What distinguishes the whole-model entry points: each extern "C" wrapper fills its own fields and leaves the rest
struct FwdOpts {
  const float* images = nullptr;      // fp32 images, or
  const uint8_t* u8 = nullptr;        // p2v_forward_u8: uint8 images in `layout`, which the input stage reads through `lut` (the rest is shared)
  int layout = 0;
  const void* lut = nullptr;
  int stop_after = -1;                // >= 0: end once that many slots of the launch numbering are filled (parity runs read the workspace)
  Prof* prof = nullptr;               // p2v_forward_profile / _begin: an event before every launch
  float *const *qkv_tap = nullptr, *const *fc1_tap = nullptr;      // p2v_forward_taps: fp32 qkv / fc1 outputs [block]
  float* const* lin_tap = nullptr;    // p2v_forward_linear_taps: fp32 output of linear layer [layer]
  DdvCtx* ddv = nullptr;              // p2v_forward_ddv / p2v_forward_stats (ddv->stats)
  bool dry = false;                   // the layout pass of p2v_forward_stats: the sequence runs, no launch is made
};

// The rows a block's launches behind the qkv GEMM run on.  ln and hid hold them compact from their start (strides D and hidden) either way.
struct RowSet {
  int rows;             // of proj, norm2, fc1 and fc2
  long long stride;     // between those rows in x and att
  int nq;               // query rows per image the attention computes (0 = all)
  bool few;             // run_gemm's few_rows, and norm2 as a launch of its own (the fused kernel is tiled over many rows)
};

// One forward in flight: what every launch needs, and the bookkeeping between launches (stop_after, profile events, taps, DDV stages)
struct Fwd {
  const p2v_plan* p;
  const FwdOpts& o;
  hipStream_t st;
  int batch, D, T, M, Hd, hd, Dk, Hk;                       // Dk, Hk: contraction depths in whole k-tiles (weights are zero-padded to them)
  int8_t *P, *X, *LN, *QKV, *ATT, *HID, *CLS;               // the workspace buffers (ws_layout)
  int launched = 0;                                         // slots of the stop_after numbering filled so far
  bool done = false;                                        // stop_after reached: a normal early end - every member is a no-op from then on

  Fwd(const p2v_plan* plan, const FwdOpts& opts, int batch_, const WsLayout& w, void* workspace, hipStream_t stream)
      : p(plan), o(opts), st(stream), batch(batch_) {
    int8_t* ws = reinterpret_cast<int8_t*>(workspace);
    P = ws + w.patches; X = ws + w.x; LN = ws + w.ln; QKV = ws + w.qkv; ATT = ws + w.att; HID = ws + w.hid; CLS = ws + w.cls;
    D = p->d.embed_dim; T = p->tokens; M = batch * T; Hd = p->d.mlp_hidden; hd = D / p->d.num_heads; Dk = round_up(D, GBK_PAD); Hk = round_up(Hd, GBK_PAD);
  }

  // One launch of kind P2V_K_*: the stop_after cut, the profile's event and kind, the launch itself, its slots
  template <class Launch>
  int step(int kind, Launch&& launch) {
    done = done || (o.stop_after >= 0 && launched >= o.stop_after);
    if (done) return P2V_OK;
    if (Prof* prof = o.prof) {
      if (prof->used + 1 >= (int)prof->ev.size()) return fail(P2V_E_LAUNCH, "profile: event pool exhausted");
      hipEventRecord(prof->ev[prof->used++], st);
      prof->kind.push_back(kind);
    }
    const int rc = o.dry ? P2V_OK : launch();
    if (rc == P2V_OK) launched += (kind == P2V_K_LN_GEMM_QKV || kind == P2V_K_LN_GEMM_FC1) ? 2 : 1;   // a fused launch fills two slots
    return rc;
  }
  // layer-output tap of p2v_forward_linear_taps: a P2V_EPI_F32 GEMM over the layer's int8 input, still in the workspace right after the
  // layer's own launch (not counted by stop_after: the entry point that passes lin_tap runs everything)
  int lin_tap(int layer, const int8_t* A, int lda, int rows, int K, int N, const p2v_linear& lin) {
    if (done || o.dry || !o.lin_tap || !o.lin_tap[layer]) return P2V_OK;
    return run_gemm(P2V_EPI_F32, A, lda, rows, K, N, lin, p2v_epilogue{}, o.lin_tap[layer], N, nullptr, st);
  }
  // a launch outside the stop_after numbering (the extra launches of the FULL stages)
  template <class Launch>
  int extra(Launch&& launch) { return o.dry ? P2V_OK : launch(); }
  // DDV stages (p2v_forward_ddv): the int8 codes a launch has just completed, fp32 values, and the fp32 tap that sits in the one tap buffer
  int ddv_i8(const void* buf, int rows, int cols, const float* scale) { return (done || !o.ddv) ? P2V_OK : ddv_reduce(o.ddv, buf, rows, cols, P2V_COS_I8, scale, st); }
  int ddv_f32(const void* buf, int rows, int cols) { return (done || !o.ddv) ? P2V_OK : ddv_reduce(o.ddv, buf, rows, cols, P2V_COS_F32, nullptr, st); }
  // codes of a QAct with per-channel (PTF) scales as the fp32 values a hook on it sees, RN(code * scale[c])
  int ddv_i8_deq(const void* buf, int rows, int cols, const float* scale) { return (done || !o.ddv) ? P2V_OK : ddv_reduce(o.ddv, buf, rows, cols, P2V_COS_I8_DEQ, scale, st); }
  int ddv_tap(int rows, int cols) { return (o.ddv && o.ddv->tap) ? ddv_f32(o.ddv->tap, rows, cols) : P2V_OK; }
  // P2V_DDV_STAGES_FULL: the stages behind the reference's remaining hook points (LayerNorm values, the mid codes of the stem and of proj / fc2)
  float* full() const { return (!done && o.ddv) ? o.ddv->scratch : nullptr; }
  int layernorm(const LnArgs& a) { return step(P2V_K_LAYERNORM, [&] { return launch_rc(p2v_launch_layernorm(a, st), "int_layernorm"); }); }
  int gemm(int kind, bool few, int epi, const int8_t* A, int lda, int rows, int K, int N, const p2v_linear& lin, const p2v_epilogue& ep, void* out, int ldo,
           int8_t* out_codes = nullptr) {
    return step(kind, [&] { return run_gemm(epi, A, lda, rows, K, N, lin, ep, out, ldo, out_codes, st, few); });
  }
  // QIntLayerNorm of `rows` rows of x -> QLinear -> `out`: one fused launch where the kernel covers the shape and the layer has fragment-order
  // weights (the LayerNorm codes then stay in LDS; parity runs read the workspace, so for them the kernel writes them too), else the
  // LayerNorm into LN and the GEMM from there
  // float LayerNorm of `rows` rows of x (pitch `stride`) into `out` (pitch D); vals: the fp32 tap or null
  int float_layernorm(const p2v_float_ln& f, long long stride, long long rows, int8_t* out, float* vals) {
    const FloatLnArgs a{X, stride, rows, D, (double)f.s_in, (double)f.eps, f.gamma, f.beta, f.g, out, D, vals};
    return step(P2V_K_LAYERNORM, [&] { return launch_rc(p2v_launch_float_layernorm(a, st), "float_layernorm"); });
  }
  // fnorm: the plan's float LayerNorm in this place, or null (QIntLayerNorm mode 'int')
  int ln_linear(int k_fused, int k_gemm, int epi, long long stride, int rows, const p2v_ln& norm, const p2v_float_ln* fnorm, const p2v_linear& lin,
                const p2v_epilogue& e, int N, int8_t* out, bool few) {
    if (fnorm) {                    // always the unfused pair: the fused LayerNorm+GEMM kernels have no float form
      float* vals = full();
      int rc = float_layernorm(*fnorm, stride, rows, LN, vals);
      if (rc || (vals && (rc = ddv_f32(vals, T, D)))) return rc;                                                 // norm1 / norm2
      return gemm(k_gemm, few, epi, LN, D, rows, Dk, N, lin, e, out, N);
    }
    LnArgs ln{X, stride, rows, D, norm, LN, D};
    ln.pre = norm.pre;
    if (float* vals = full()) {     // FULL DDV stages: the unfused pair, the LayerNorm's values reduced before the GEMM's tap reuses the buffer
      ln.tap_out = vals;
      int rc = layernorm(ln);
      if (rc || (rc = ddv_f32(vals, T, D))) return rc;                                                           // norm1 / norm2
      return gemm(k_gemm, few, epi, LN, D, rows, Dk, N, lin, e, out, N);
    }
    if (!few && lin.w_frag && p2v_ln_gemm_supported(epi, D, N, e.gelu.table ? e.gelu.cells : 0)) {
      if (o.stop_after < 0) ln.out = nullptr;
      return step(k_fused, [&] { return run_ln_gemm(epi, ln, lin, e, N, out, st); });
    }
    const int rc = layernorm(ln);
    return rc ? rc : gemm(k_gemm, few, epi, LN, D, rows, Dk, N, lin, e, out, N);
  }

  // Block i on the rows `rs` names; bc: its four bit widths (qkv, proj, fc1, fc2).  The taps and DDV stages name whole [T][..] samples: the
  // entry points that ask for them run every block on all rows.
  int block(int i, const int8_t* bc, const RowSet& rs) {
    const p2v_block& b = p->blocks[i];
    const int bq = bit_index(bc[0]), bp = bit_index(bc[1]), b1 = bit_index(bc[2]), b2 = bit_index(bc[3]);
    const p2v_linear &qkv = p->lin[bq][1 + 4 * i], &proj = p->lin[bp][2 + 4 * i], &fc1 = p->lin[b1][3 + 4 * i], &fc2 = p->lin[b2][4 + 4 * i];
    const int ldx = (int)rs.stride;
    int rc;
    // norm1 -> /channel_scale -> qact0 -> qkv -> qact1, every row (the keys and values)       vit_fquant.py:431-434,284-293,307
    p2v_epilogue eq{};
    eq.inv_s_out = b.inv_s_qkv[bq];
    eq.tap_out = o.qkv_tap ? o.qkv_tap[i] : (o.lin_tap ? o.lin_tap[1 + 4 * i] : nullptr);
    const p2v_float_block& fb = p->fblocks[i];
    if ((rc = ln_linear(P2V_K_LN_GEMM_QKV, P2V_K_GEMM_QKV, P2V_EPI_REQUANT, D, M, b.ln1[bq], p->float_norm ? &fb.ln1[bq] : nullptr, qkv, eq, 3 * D, QKV,
                        false)))
      return rc;
    if ((rc = ddv_tap(T, 3 * D)) || (rc = ddv_i8(QKV, T, 3 * D, nullptr))) return rc;                           // attn.qkv, attn.qact1
    // scores -> qact_attn1 -> log-int-softmax -> @v -> qact2                  vit_fquant.py:309-326
    if (p->float_softmax) {        // scores -> qact_attn1 -> softmax (table) -> @v -> qact2
      const SmAttnArgs sa{QKV, batch, T, p->d.num_heads, b.attn.s_qkv_sq, b.attn.qk_scale, b.attn.inv_s_attn, b.attn.av_mul, fb.softmax_table, ATT, nullptr, 0, rs.nq};
      if ((rc = step(P2V_K_ATTENTION, [&] { return launch_rc(p2v_launch_softmax_attention(sa, hd, st), "softmax_attention"); }))) return rc;
    } else {
      AttnArgs at{{QKV, batch, T, p->d.num_heads, b.attn, ATT, nullptr}};
      at.nq = rs.nq;
      at.klim = 1 << p->softmax_bits[i];
      int8_t* planes = (!done && o.ddv) ? o.ddv->attn : nullptr;              // P2V_DDV_STAGES_ATTN: the tapped launch, both planes of this block
      const int pitch = round_up(T, 16), HT = p->d.num_heads * T;
      if (planes) {
        at.score_codes = planes;
        at.probs_kp = planes + (size_t)batch * HT * pitch;
        at.pitch = pitch;
      }
      if ((rc = step(P2V_K_ATTENTION, [&] { return launch_rc(p2v_launch_attention(at, hd, st), "lis_attention"); }))) return rc;
      if (planes && !done &&
          ((rc = ddv_reduce(o.ddv, at.score_codes, HT, T, P2V_COS_I8, nullptr, st, 0, pitch)) ||                      // attn.qact_attn1
           (rc = ddv_reduce(o.ddv, at.probs_kp, HT, T, P2V_COS_LOG2K, nullptr, st, 0, pitch))))                        // attn.log_int_softmax
        return rc;
    }
    if ((rc = ddv_i8(ATT, T, D, nullptr))) return rc;                                                            // attn.qact2
    // proj -> qact3 -> + x -> Block.qact2, in place on x                      vit_fquant.py:334-338,431
    p2v_epilogue ep = b.proj_epi;
    ep.residual = X;
    ep.resid_tab = p->resid_tab[(size_t)i * 4 + bp];
    // (FULL DDV stages: the codes of attn.qact3 go to ln, which nothing reads between norm1's GEMM and norm2)
    if ((rc = gemm(P2V_K_GEMM_PROJ, rs.few, P2V_EPI_RESID, ATT, ldx, rs.rows, Dk, D, proj, ep, X, ldx, full() ? LN : nullptr))) return rc;
    if ((rc = lin_tap(2 + 4 * i, ATT, ldx, rs.rows, Dk, D, proj)) || (rc = ddv_tap(T, D))) return rc;            // attn.proj
    if (full() && (rc = ddv_i8_deq(LN, T, D, b.proj_epi.s_mid))) return rc;                                      // attn.qact3
    if ((rc = ddv_i8(X, T, D, b.proj_epi.s_next))) return rc;                                                    // Block.qact2
    // norm2 (attention's channel scale!) -> /mlp.channel_scale -> mlp.qact0 -> fc1 -> GELU -> qact1     vit_fquant.py:464, layers_quant.py:305-316,331-333
    p2v_epilogue e1{};
    e1.inv_s_out = b.inv_s_fc1;
    e1.gelu = b.gelu_fc1;
    e1.tap_out = o.fc1_tap ? o.fc1_tap[i] : (o.lin_tap ? o.lin_tap[3 + 4 * i] : nullptr);
    if ((rc = ln_linear(P2V_K_LN_GEMM_FC1, P2V_K_GEMM_FC1, P2V_EPI_GELU, rs.stride, rs.rows, b.ln2[bq][b1], p->float_norm ? &fb.ln2[bq][b1] : nullptr, fc1, e1,
                        Hd, HID, rs.few)))
      return rc;
    if ((rc = ddv_tap(T, Hd)) || (rc = ddv_i8(HID, T, Hd, nullptr))) return rc;                                 // mlp.fc1, mlp.qact1
    // fc2 -> qact2 -> + x -> Block.qact4, in place on x                       layers_quant.py:342-346, vit_fquant.py:468
    p2v_epilogue e2 = b.fc2_epi;
    e2.residual = X;
    e2.resid_tab = p->resid_tab[(size_t)i * 4 + 2 + b2];
    if ((rc = gemm(P2V_K_GEMM_FC2, rs.few, P2V_EPI_RESID, HID, Hd, rs.rows, Hk, D, fc2, e2, X, ldx, full() ? LN : nullptr))) return rc;
    if ((rc = lin_tap(4 + 4 * i, HID, Hd, rs.rows, Hk, D, fc2)) || (rc = ddv_tap(T, D))) return rc;             // mlp.fc2
    if (full() && (rc = ddv_i8_deq(LN, T, D, b.fc2_epi.s_mid))) return rc;                                       // mlp.qact2
    return ddv_i8(X, T, D, b.fc2_epi.s_next);                                                                    // Block.qact4
  }

  // The pieces of a forward, in the order forward_impl runs them: stem, block_at 0 .. depth - 1, final_norm, head, finish.  Of the workspace
  // only x carries state from one piece to the next (cls: from final_norm to head), which is what p2v_forward_many's shared prefixes rest on.
  int stem(int bits);
  int block_at(int i, const int8_t* bc);
  int final_norm();
  int head(int bits, float* logits);
  int finish();
};

// What every whole-model entry point asks of a bit list and of the plan it runs on (before any HIP call)
static int check_forward(const p2v_plan* p, const int8_t* bit_config, int n_cfg, const FwdOpts& o) {
  if (n_cfg != p->n_layers) return fail(P2V_E_BITS, "bit_config has %d entries, model needs %d", n_cfg, p->n_layers);
  for (int i = 0; i < n_cfg; ++i) {
    const int bi = bit_index(bit_config[i]);
    if (bi < 0) return fail(P2V_E_BITS, "%d is not in list", (int)bit_config[i]);   // bit_pool.index, vit_fquant.py:282
    if (!p->lin_set[bi][i]) return fail(P2V_E_STATE, "layer %d has no %d-bit weights", i, (int)bit_config[i]);
  }
  if (!p->embed_set || !p->head_set) return fail(P2V_E_STATE, "plan incomplete (embed/head)");
  for (int i = 0; i < p->d.depth; ++i)
    if (!p->block_set[i]) return fail(P2V_E_STATE, "plan incomplete (block %d)", i);
  if (p->float_norm || p->float_softmax) {
    for (int i = 0; i < p->d.depth; ++i)
      if (!p->fblock_set[i]) return fail(P2V_E_STATE, "plan incomplete (float operators of block %d: p2v_plan_set_float_block)", i);
    if (p->float_norm && !p->fhead_set) return fail(P2V_E_STATE, "plan incomplete (float final norm: p2v_plan_set_float_head)");
    if (p->float_softmax && o.ddv && o.ddv->attn)
      return fail(P2V_E_UNSUPPORTED, "P2V_DDV_STAGES_ATTN: the plan's softmax is the float one, its probabilities are not codes");
  }
  return P2V_OK;
}

// qact_input + PatchEmbed + cls/pos/qact1 into x, every row of it; bits: the convolution's width      vit_fquant.py:705-733
int Fwd::stem(int bits) {
  Fwd& f = *this;
  const p2v_model_desc& d = p->d;
  const int Kp = p->k_patch_pad, rows_p = batch * p->patches;
  int rc;
  const p2v_linear& embed = p->lin[bit_index(bits)][0];
  if (p->inv_s_input > 0.f) {
    rc = f.step(P2V_K_PATCHIFY, [&] {
      return o.u8 ? launch_rc(p2v_launch_u8_patchify(o.u8, batch, d.in_chans, d.img_size, d.img_size, d.patch_size, o.layout, (const int8_t*)o.lut, f.P, Kp, st), "u8_patchify")
                  : launch_rc(p2v_launch_patchify(o.images, batch, d.in_chans, d.img_size, d.img_size, d.patch_size, p->inv_s_input, f.P, Kp, st), "quantize_patchify");
    });
    if (rc) return rc;
    if (f.full()) {
      // FULL DDV stages of the stem: the patch matrix (qact_input: a permutation of the image's codes plus zero columns), then the EMBED launch
      // with its two mid-code planes in qkv (free until block 0), both [M][D] in the token layout of x: patch_embed.qact over the patch rows,
      // qact_embed over all rows once the constant class row is filled in
      int8_t *pe = f.QKV, *em = f.QKV + (size_t)f.M * D;
      GemmArgs g = gemm_args(f.P, Kp, rows_p, embed.w_codes, Kp, D, embed, p->embed_epi, f.X, D, pe);
      g.out_codes2 = em;
      // (the statistics take the real C * P^2 columns of the patch matrix, not the zero columns up to k_pad; a cosine does not see those)
      const int Kc = o.ddv->stats ? d.in_chans * d.patch_size * d.patch_size : Kp;
      if ((rc = ddv_reduce(o.ddv, f.P, p->patches, Kc, P2V_COS_I8, nullptr, st, (long long)p->patches * Kp, Kp)) ||   // qact_input
          (rc = f.step(P2V_K_GEMM_EMBED, [&] { return launch_rc(p2v_launch_gemm(P2V_EPI_EMBED, g, st), "gemm_i8"); })) ||
          (rc = ddv_reduce(o.ddv, pe + D, p->patches, D, P2V_COS_I8, nullptr, st, (long long)T * D)) ||           // patch_embed.qact
          (rc = f.extra([&] { return launch_rc(p2v_launch_fill_cls(em, batch, T, D, p->embed_cls_codes, st), "fill_cls"); })) ||
          (rc = f.ddv_i8(em, T, D, nullptr)))                                                                     // qact_embed
        return rc;
    } else if ((rc = f.gemm(P2V_K_GEMM_EMBED, false, P2V_EPI_EMBED, f.P, Kp, rows_p, Kp, D, embed, p->embed_epi, f.X, D))) {
      return rc;
    }
    if ((rc = f.lin_tap(0, f.P, Kp, rows_p, Kp, D, embed))) return rc;
  } else {
    // input_quant = False (vit_fquant.py:705, the vit_large factory :925): the fp32 image feeds the fake-quantised convolution
    if (embed.packed4) return fail(P2V_E_UNSUPPORTED, "input_quant = False: the patch-embed weights must be unpacked codes (packed4 = 0)");
    const GemmArgs g = gemm_args(nullptr, 0, rows_p, embed.w_codes, Kp, D, embed, p->embed_epi, f.X, D, nullptr);
    rc = f.step(P2V_K_GEMM_EMBED, [&] {
      return o.u8 ? launch_rc(p2v_launch_embed_u8(o.u8, o.layout, (const float*)o.lut, batch, d.in_chans, d.img_size, d.img_size, d.patch_size, g, st), "embed_u8")
                  : launch_rc(p2v_launch_embed_fp32(o.images, batch, d.in_chans, d.img_size, d.img_size, d.patch_size, g, st), "embed_fp32");
    });
    if (rc) return rc;
  }
  if ((rc = f.step(P2V_K_FILL_CLS, [&] { return launch_rc(p2v_launch_fill_cls(f.X, batch, T, D, p->cls_codes, st), "fill_cls"); })))
    return rc;
  return f.ddv_i8(f.X, T, D, p->embed_epi.s_next);                                                               // qact1
}

// Block i of the forward on the rows it needs; bc: its four bit widths
int Fwd::block_at(int i, const int8_t* bc) {
  // The logits read the last block's output through its class-token rows only (the final norm below takes [:, 0]) and everything
  // behind the qkv GEMM is row-local but for the attention's keys and values: query row 0 of every (image, head), then proj, norm2,
  // fc1 and fc2 on `batch` rows - proj and fc2 in place on the class rows of x (stride T * D), the rows between them compact at the
  // start of ln / hid.  The patch rows of x / att / hid keep what the launches before left there.  So the last block runs on the class
  // rows when nothing but the logits is asked for (parity runs read the workspace), and T * D fits the int strides of a GEMM.
  const bool cls_only = g_cls_rows && !p->float_norm && !p->float_softmax && o.stop_after < 0 && !o.qkv_tap && !o.fc1_tap && !o.lin_tap && !o.ddv && (long long)T * D <= 0x7fffffffLL;
  const RowSet all_rows{M, D, 0, false}, cls_rows{batch, (long long)T * D, 1, true};
  return block(i, bc, (cls_only && i == p->d.depth - 1) ? cls_rows : all_rows);
}

// norm over the cls rows only ([:,0]) -> qact2, into cls; x stays as it is                             vit_fquant.py:766-767
int Fwd::final_norm() {
  Fwd& f = *this;
  int rc;
  if (p->float_norm) {
    if (float* vals = f.full()) {    // FULL DDV stages: the final norm once more, over every row, for its values
      const FloatLnArgs a{f.X, D, f.M, D, (double)p->final_fln.s_in, (double)p->final_fln.eps, p->final_fln.gamma, p->final_fln.beta, p->final_fln.g, f.LN, D, vals};
      if ((rc = f.extra([&] { return launch_rc(p2v_launch_float_layernorm(a, st), "float_layernorm"); })) || (rc = f.ddv_f32(vals, T, D))) return rc;   // norm
    }
    if ((rc = f.float_layernorm(p->final_fln, (long long)T * D, batch, f.CLS, nullptr)) || (rc = f.ddv_i8(f.CLS, 1, D, nullptr))) return rc;   // qact2
  } else {
    if (float* vals = f.full()) {      // FULL DDV stages: the hook on `norm` sits in front of [:, 0] - the final norm once more, over every row (codes into ln)
      LnArgs la{f.X, D, f.M, D, p->final_ln, f.LN, D};
      la.pre = p->final_ln.pre;
      la.tap_out = vals;
      if ((rc = f.extra([&] { return launch_rc(p2v_launch_layernorm(la, st), "int_layernorm"); })) || (rc = f.ddv_f32(vals, T, D))) return rc;   // norm
    }
    LnArgs lf{f.X, (long long)T * D, batch, D, p->final_ln, f.CLS, D};
    lf.pre = p->final_ln.pre;
    if ((rc = f.layernorm(lf)) || (rc = f.ddv_i8(f.CLS, 1, D, nullptr))) return rc;                               // qact2
  }
  return P2V_OK;
}

// head -> act_out: cls -> logits; bits: the head's width                                               vit_fquant.py:790-796
int Fwd::head(int bits, float* logits) {
  Fwd& f = *this;
  const p2v_model_desc& d = p->d;
  const int n_cfg = p->n_layers;
  int rc;
  const p2v_linear& lin = p->lin[bit_index(bits)][n_cfg - 1];
  p2v_epilogue eh{};
  eh.inv_s_out = p->head_inv_s;
  eh.s_out = p->head_s;
  if ((rc = f.gemm(P2V_K_GEMM_HEAD, false, P2V_EPI_HEAD, f.CLS, D, batch, f.Dk, d.num_classes, lin, eh, logits, d.num_classes))) return rc;
  if ((rc = f.lin_tap(n_cfg - 1, f.CLS, D, batch, f.Dk, d.num_classes, lin)) || (rc = f.ddv_tap(1, d.num_classes))) return rc;   // head
  return f.ddv_f32(logits, 1, d.num_classes);                                                                    // act_out
}

// the end of a whole pass: the profile's closing events
int Fwd::finish() {
  Fwd& f = *this;
  if (f.done) return P2V_OK;
  if (Prof* prof = o.prof) {
    if (prof->used + 2 > (int)prof->ev.size()) return fail(P2V_E_LAUNCH, "profile: event pool exhausted");
    hipEventRecord(prof->ev[prof->used++], st);
    hipEventRecord(prof->ev[prof->used++], st);      // an empty interval: the cost of the event pair itself (P2V_K_EVENT_GAP)
    prof->kind.push_back(P2V_K_EVENT_GAP);
  }
  return P2V_OK;
}

static int forward_impl(p2v_plan* p, int batch, const int8_t* bit_config, int n_cfg, float* logits, void* workspace, size_t workspace_bytes,
                        void* stream, const FwdOpts& o) {
  if (!p || !(o.images || o.u8) || !bit_config || !logits || !workspace) return fail(P2V_E_ARG, "p2v_forward: null argument");
  if (batch <= 0) return fail(P2V_E_SHAPE, "batch must be positive");
  if (const int rc = check_forward(p, bit_config, n_cfg, o)) return rc;
  const WsLayout w = ws_layout(p, batch);
  if (workspace_bytes < w.total) return fail(P2V_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, w.total);
  if (o.lin_tap && o.lin_tap[0] && !(p->inv_s_input > 0.f))
    return fail(P2V_E_UNSUPPORTED, "p2v_forward_linear_taps: no patch-embed tap for input_quant = False (the fp32-image convolution); pass NULL for taps[0]");
  Fwd f(p, o, batch, w, workspace, (hipStream_t)stream);
  int rc;
  if ((rc = f.stem(bit_config[0]))) return rc;
  for (int i = 0; i < p->d.depth && !f.done; ++i)
    if ((rc = f.block_at(i, bit_config + 1 + 4 * i))) return rc;
  if ((rc = f.final_norm()) || (rc = f.head(bit_config[n_cfg - 1], logits))) return rc;
  return f.finish();
}

// ---- p2v_forward_many: several bit lists in one call --------------------------------------------------------------------------------------
// A prefix tree over the lists, depth + 2 levels deep: level 0 is keyed by the stem's entry, level 1 + i by the four entries of block i, the
// last one is the tail (the final norm once, then a head GEMM per distinct head entry).  The walk is depth first, the children of a node in
// the order the caller's array first shows them; what the lists of a node share has run once when the walk reaches it.  A node with several
// children keeps x in a snapshot slot (saved once, restored in front of every child but the first): x is all a block hands to the next, and
// the engine is integer-exact, so a list's logits are those of a forward of its own.  The stem writes every row of x and the tail writes none
// of it: the root and the tail need no slot.  The same walk with f == nullptr only counts (p2v_forward_many_plan, p2v_forward_many_bytes).
struct ManyWalk {
  const int8_t* cfgs;                 // host [n_lists][n_cfg]
  int n_cfg, depth;
  Fwd* f = nullptr;
  float* logits = nullptr;            // dev [n_lists][per_list]
  size_t per_list = 0;                // batch * classes
  int8_t* slots = nullptr;            // the snapshot slots, slot_bytes apart; x_bytes of each are used
  size_t slot_bytes = 0, x_bytes = 0;
  int stems = 0, blocks = 0, norms = 0, heads = 0, copies = 0, snapshots = 0;

  // the entries of list l that level `level` is keyed by, as one word (a level has at most four of them)
  uint32_t key(int l, int level) const {
    const int8_t* c = cfgs + (size_t)l * n_cfg;
    const int lo = level == 0 ? 0 : (level <= depth ? 1 + 4 * (level - 1) : n_cfg - 1), n = (level >= 1 && level <= depth) ? 4 : 1;
    uint32_t k = 0;
    memcpy(&k, c + lo, n);
    return k;
  }
  // `lists` by their key of `level`, groups and members in order of first appearance
  std::vector<std::vector<int>> children(const std::vector<int>& lists, int level) const {
    std::vector<std::vector<int>> groups;
    std::vector<uint32_t> keys;
    for (int l : lists) {
      const uint32_t k = key(l, level);
      size_t g = 0;
      while (g < keys.size() && keys[g] != k) ++g;
      if (g == keys.size()) {
        keys.push_back(k);
        groups.emplace_back();
      }
      groups[g].push_back(l);
    }
    return groups;
  }
  int copy(void* dst, const void* src, size_t bytes) {
    if (!f) return P2V_OK;
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, f->st);
    return e == hipSuccess ? P2V_OK : fail(P2V_E_LAUNCH, "p2v_forward_many: hipMemcpyAsync: %s", hipGetErrorString(e));
  }
  // the final norm of the lists' common x, a head GEMM per distinct head entry, a copy of the logits per repeated list
  int tail(const std::vector<int>& lists) {
    int rc;
    ++norms;
    if (f && (rc = f->final_norm())) return rc;
    for (const std::vector<int>& g : children(lists, depth + 1)) {
      float* out = logits + (size_t)g[0] * per_list;
      ++heads;
      if (f && (rc = f->head(cfgs[(size_t)g[0] * n_cfg + n_cfg - 1], out))) return rc;
      for (size_t k = 1; k < g.size(); ++k)
        if ((rc = copy(logits + (size_t)g[k] * per_list, out, per_list * sizeof(float)))) return rc;
    }
    return P2V_OK;
  }
  // `lists` agree on every level in front of `level`, whose launches have run; `held`: the snapshot slots in use on the way here
  int visit(const std::vector<int>& lists, int level, int held) {
    if (level == depth + 1) return tail(lists);
    const std::vector<std::vector<int>> groups = children(lists, level);
    const bool keep = level > 0 && groups.size() > 1;
    int8_t* slot = f ? slots + (size_t)held * slot_bytes : nullptr;
    int rc;
    if (keep) {
      snapshots = snapshots > held + 1 ? snapshots : held + 1;
      ++copies;
      if (f && (rc = copy(slot, f->X, x_bytes))) return rc;
    }
    for (size_t g = 0; g < groups.size(); ++g) {
      const int8_t* c = cfgs + (size_t)groups[g][0] * n_cfg;
      if (keep && g > 0) {
        ++copies;
        if (f && (rc = copy(f->X, slot, x_bytes))) return rc;
      }
      if (level == 0) {
        ++stems;
        if (f && (rc = f->stem(c[0]))) return rc;
      } else {
        ++blocks;
        if (f && (rc = f->block_at(level - 1, c + 1 + 4 * (level - 1)))) return rc;
      }
      if ((rc = visit(groups[g], level + 1, held + (keep ? 1 : 0)))) return rc;
    }
    return P2V_OK;
  }
  int run(int n_lists) {
    std::vector<int> all(n_lists);
    for (int l = 0; l < n_lists; ++l) all[l] = l;
    return visit(all, 0, 0);
  }
};

// what the three p2v_forward_many* entry points ask of the lists; the plan only has to exist
static int check_many_lists(const char* who, const p2v_plan* p, const int8_t* bit_configs, int n_lists, int n_cfg) {
  if (!p || !bit_configs) return fail(P2V_E_ARG, "%s: null argument", who);
  if (n_lists < 1 || n_lists > P2V_MANY_MAX_LISTS) return fail(P2V_E_SHAPE, "%s: %d lists (1 ... %d are taken)", who, n_lists, P2V_MANY_MAX_LISTS);
  if (n_cfg != p->n_layers) return fail(P2V_E_BITS, "%s: the bit lists have %d entries, model needs %d", who, n_cfg, p->n_layers);
  for (int l = 0; l < n_lists; ++l)
    for (int i = 0; i < n_cfg; ++i)
      if (bit_index(bit_configs[(size_t)l * n_cfg + i]) < 0)
        return fail(P2V_E_BITS, "%s: list %d: %d is not in list", who, l, (int)bit_configs[(size_t)l * n_cfg + i]);
  return P2V_OK;
}
static size_t many_slot_bytes(const p2v_plan* p, int batch) { return ((size_t)batch * p->tokens * p->d.embed_dim + 255) / 256 * 256; }

static int forward_many_impl(const char* who, p2v_plan* p, int batch, const int8_t* bit_configs, int n_lists, int n_cfg, float* logits, void* ws,
                             size_t ws_bytes, void* stream, const FwdOpts& o) {
  if (!p || !(o.images || o.u8) || !bit_configs || !logits || !ws) return fail(P2V_E_ARG, "%s: null argument", who);
  if (batch <= 0) return fail(P2V_E_SHAPE, "%s: batch must be positive", who);
  int rc;
  if ((rc = check_many_lists(who, p, bit_configs, n_lists, n_cfg))) return rc;
  for (int l = 0; l < n_lists; ++l)
    if ((rc = check_forward(p, bit_configs + (size_t)l * n_cfg, n_cfg, o))) {
      char why[sizeof g_err];
      memcpy(why, g_err, sizeof why);
      return fail(rc, "%s: list %d: %.400s", who, l, why);
    }
  ManyWalk dry{bit_configs, n_cfg, p->d.depth};
  dry.run(n_lists);
  const WsLayout w = ws_layout(p, batch);
  const size_t need = w.total + (size_t)dry.snapshots * many_slot_bytes(p, batch);
  if (ws_bytes < need) return fail(P2V_E_WORKSPACE, "%s: workspace %zu < %zu bytes (p2v_forward_many_bytes)", who, ws_bytes, need);
  Fwd f(p, o, batch, w, ws, (hipStream_t)stream);
  ManyWalk walk{bit_configs, n_cfg, p->d.depth};
  walk.f = &f;
  walk.logits = logits;
  walk.per_list = (size_t)batch * p->d.num_classes;
  walk.slots = reinterpret_cast<int8_t*>(ws) + w.total;
  walk.slot_bytes = many_slot_bytes(p, batch);
  walk.x_bytes = (size_t)batch * p->tokens * p->d.embed_dim;
  return walk.run(n_lists);
}

extern "C" {

int p2v_forward(p2v_plan* p, const float* images, int batch, const int8_t* bit_config, int n_cfg, float* logits, void* workspace,
                size_t workspace_bytes, int stop_after, void* stream) {
  FwdOpts o;
  o.images = images; o.stop_after = stop_after;
  return forward_impl(p, batch, bit_config, n_cfg, logits, workspace, workspace_bytes, stream, o);
}

int p2v_forward_many_plan(const p2v_plan* plan, const int8_t* bit_configs, int n_lists, int n_cfg, int* stems, int* blocks, int* norms, int* heads,
                          int* copies, int* snapshots) {
  if (const int rc = check_many_lists("p2v_forward_many_plan", plan, bit_configs, n_lists, n_cfg)) return rc;
  ManyWalk w{bit_configs, n_cfg, plan->d.depth};
  w.run(n_lists);
  const struct { int* out; int v; } counts[] = {{stems, w.stems}, {blocks, w.blocks}, {norms, w.norms}, {heads, w.heads}, {copies, w.copies},
                                                {snapshots, w.snapshots}};
  for (const auto& c : counts)
    if (c.out) *c.out = c.v;
  return P2V_OK;
}

size_t p2v_forward_many_bytes(const p2v_plan* plan, int batch, const int8_t* bit_configs, int n_lists, int n_cfg) {
  int snapshots = 0;
  if (!plan || batch <= 0 || p2v_forward_many_plan(plan, bit_configs, n_lists, n_cfg, nullptr, nullptr, nullptr, nullptr, nullptr, &snapshots)) return 0;
  return ws_layout(plan, batch).total + (size_t)snapshots * many_slot_bytes(plan, batch);
}

int p2v_forward_many(p2v_plan* p, const float* images, int batch, const int8_t* bit_configs, int n_lists, int n_cfg, float* logits, void* ws,
                     size_t ws_bytes, void* stream) {
  FwdOpts o;
  o.images = images;
  return forward_many_impl("p2v_forward_many", p, batch, bit_configs, n_lists, n_cfg, logits, ws, ws_bytes, stream, o);
}

// uint8 input (p2v_forward_u8, p2v_u8_patchify): images and table present, a known layout, images 4-byte aligned (the kernels read dwords)
static int check_u8_input(const char* what, const uint8_t* img, int layout, const void* lut) {
  if (!img || !lut) return fail(P2V_E_ARG, "%s: null images or lut", what);
  if (layout != P2V_LAYOUT_NCHW && layout != P2V_LAYOUT_NHWC) return fail(P2V_E_ARG, "%s: unknown layout %d (P2V_LAYOUT_NCHW = 0, NHWC = 1)", what, layout);
  if (reinterpret_cast<uintptr_t>(img) & 3) return fail(P2V_E_ARG, "%s: images must start on a 4-byte boundary", what);
  return P2V_OK;
}

int p2v_forward_u8(p2v_plan* p, const uint8_t* images, int layout, const void* lut, int batch, const int8_t* bit_config, int n_cfg,
                   float* logits, void* workspace, size_t workspace_bytes, int stop_after, void* stream) {
  const int rc = check_u8_input("p2v_forward_u8", images, layout, lut);
  if (rc) return rc;
  FwdOpts o;
  o.u8 = images; o.layout = layout; o.lut = lut; o.stop_after = stop_after;
  return forward_impl(p, batch, bit_config, n_cfg, logits, workspace, workspace_bytes, stream, o);
}

int p2v_forward_many_u8(p2v_plan* p, const uint8_t* images, int layout, const void* lut, int batch, const int8_t* bit_configs, int n_lists,
                        int n_cfg, float* logits, void* ws, size_t ws_bytes, void* stream) {
  const int rc = check_u8_input("p2v_forward_many_u8", images, layout, lut);
  if (rc) return rc;
  FwdOpts o;
  o.u8 = images; o.layout = layout; o.lut = lut;
  return forward_many_impl("p2v_forward_many_u8", p, batch, bit_configs, n_lists, n_cfg, logits, ws, ws_bytes, stream, o);
}

int p2v_forward_taps(p2v_plan* p, const float* images, int batch, const int8_t* bit_config, int n_cfg, float* logits, void* workspace,
                     size_t workspace_bytes, float* const* qkv_out, float* const* fc1_out, void* stream) {
  FwdOpts o;
  o.images = images; o.qkv_tap = qkv_out; o.fc1_tap = fc1_out;
  return forward_impl(p, batch, bit_config, n_cfg, logits, workspace, workspace_bytes, stream, o);
}

int p2v_forward_linear_taps(p2v_plan* p, const float* images, int batch, const int8_t* bit_config, int n_cfg, float* logits, void* ws,
                            size_t ws_bytes, float* const* taps, void* stream) {
  if (!taps) return fail(P2V_E_ARG, "p2v_forward_linear_taps: null taps array");
  FwdOpts o;
  o.images = images; o.lin_tap = taps;
  return forward_impl(p, batch, bit_config, n_cfg, logits, ws, ws_bytes, stream, o);
}

static int prof_collect(Prof& prof, float* ms_out, int32_t* kind_out, int max_launches) {
  hipEventSynchronize(prof.ev[prof.used - 1]);
  int n = (int)prof.kind.size();
  n = n < max_launches ? n : max_launches;          // never more than the caller's arrays hold
  for (int i = 0; i < n; ++i) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, prof.ev[i], prof.ev[i + 1]);
    ms_out[i] = ms;
    kind_out[i] = prof.kind[i];
  }
  return n;
}

int p2v_forward_profile_begin(p2v_plan* p, const float* images, int batch, const int8_t* bit_config, int n_cfg, float* logits, void* workspace,
                              size_t workspace_bytes, void* stream, void** token) {
  if (!p || !token) return fail(P2V_E_ARG, "p2v_forward_profile_begin: null argument");
  *token = nullptr;
  if (const int cap = refuse_capture("p2v_forward_profile_begin", "times every launch with events of its own", stream)) return cap;
  std::unique_ptr<Prof> prof(new Prof());
  if (!prof->make_pool(prof_pool_size(p))) return fail(P2V_E_LAUNCH, "hipEventCreate failed");
  prof->st = (hipStream_t)stream;
  FwdOpts o;
  o.images = images; o.prof = prof.get();
  const int rc = forward_impl(p, batch, bit_config, n_cfg, logits, workspace, workspace_bytes, stream, o);
  if (rc == P2V_OK) *token = prof.release();        // the caller's, until p2v_forward_profile_end
  return rc;
}

int p2v_forward_profile_end(void* token, float* ms_out, int32_t* kind_out, int max_launches) {
  if (!token) return fail(P2V_E_ARG, "p2v_forward_profile_end: null argument");
  Prof* prof = reinterpret_cast<Prof*>(token);
  // (the token stays the caller's: it is ended once the capture is over)
  if (const int cap = refuse_capture("p2v_forward_profile_end", "waits for the last event of the pass; the token stays valid", prof->st)) return cap;
  int n = 0;
  if (ms_out && kind_out && max_launches > 0) n = prof_collect(*prof, ms_out, kind_out, max_launches);
  else hipEventSynchronize(prof->ev[prof->used - 1]);      // ms_out == NULL: just release the token (error paths of the caller)
  delete prof;
  return n;
}

int p2v_forward_profile(p2v_plan* p, const float* images, int batch, const int8_t* bit_config, int n_cfg, float* logits, void* workspace,
                        size_t workspace_bytes, void* stream, float* ms_out, int32_t* kind_out, int max_launches) {
  if (!p || !ms_out || !kind_out || max_launches <= 0) return fail(P2V_E_ARG, "p2v_forward_profile: null argument");
  if (const int cap = refuse_capture("p2v_forward_profile", "times every launch with events and waits for the last one", stream)) return cap;
  void* token;
  const int rc = p2v_forward_profile_begin(p, images, batch, bit_config, n_cfg, logits, workspace, workspace_bytes, stream, &token);
  return rc == P2V_OK ? p2v_forward_profile_end(token, ms_out, kind_out, max_launches) : rc;
}

// ---- per-operator entry points ------------------------------------------------------------------------
// what both patchify entry points ask of the image and of the patch matrix's row
static int check_patchify_shape(int chans, int height, int width, int patch, int k_pad) {
  if (patch <= 0 || patch % 4 || height % patch || width % patch) return fail(P2V_E_SHAPE, "image %dx%d not divisible into %d-patches", height, width, patch);
  if (k_pad % 4 || k_pad < chans * patch * patch) return fail(P2V_E_ARG, "k_pad %d too small / unaligned", k_pad);
  return P2V_OK;
}

int p2v_quantize_patchify(const float* img, int batch, int chans, int height, int width, int patch, float inv_s, int8_t* out,
                          int k_pad, void* stream) {
  if (!img || !out) return fail(P2V_E_ARG, "p2v_quantize_patchify: null argument");
  if (const int rc = check_patchify_shape(chans, height, width, patch, k_pad)) return rc;
  return launch_rc(p2v_launch_patchify(img, batch, chans, height, width, patch, inv_s, out, k_pad, (hipStream_t)stream), "quantize_patchify");
}

int p2v_u8_patchify(const uint8_t* img, int layout, const void* lut_i8, int batch, int chans, int height, int width, int patch, int8_t* out,
                    int k_pad, void* stream) {
  int rc = check_u8_input("p2v_u8_patchify", img, layout, lut_i8);
  if (rc) return rc;
  if (!out) return fail(P2V_E_ARG, "p2v_u8_patchify: null argument");
  if (batch <= 0 || chans <= 0) return fail(P2V_E_SHAPE, "p2v_u8_patchify: batch %d, %d channels", batch, chans);
  if ((rc = check_patchify_shape(chans, height, width, patch, k_pad))) return rc;
  return launch_rc(p2v_launch_u8_patchify(img, batch, chans, height, width, patch, layout, (const int8_t*)lut_i8, out, k_pad, (hipStream_t)stream),
                   "u8_patchify");
}

int p2v_gemm_i8(int kind, const int8_t* A, int lda, int M, int K, int N, const p2v_linear* lin, const p2v_epilogue* epi, void* out,
                int ldo, int8_t* out_codes, void* stream) {
  if (!A || !lin || !epi || !out) return fail(P2V_E_ARG, "p2v_gemm_i8: null argument");
  if (kind < P2V_EPI_REQUANT || kind > P2V_EPI_HEAD) return fail(P2V_E_ARG, "unknown epilogue %d", kind);
  if (M <= 0 || N <= 0 || K <= 0 || K % GBK_PAD) return fail(P2V_E_SHAPE, "K=%d must be a positive multiple of %d", K, GBK_PAD);
  if (kind != P2V_EPI_HEAD && (N % 16 || ldo % 16)) return fail(P2V_E_UNSUPPORTED, "N and ldo must be multiples of 16 for int8 outputs");
  if (lda % 16) return fail(P2V_E_UNSUPPORTED, "lda must be a multiple of 16");
  if (lda <= 0 || ldo < N) return fail(P2V_E_SHAPE, "p2v_gemm_i8: lda=%d must be positive and ldo=%d must cover the %d outputs of a row", lda, ldo, N);
  if (kind == P2V_EPI_REQUANT && check_requant_scale("p2v_gemm_i8", epi->inv_s_out) != P2V_OK) return P2V_E_UNSUPPORTED;
  if (kind == P2V_EPI_GELU && check_gelu_tab("p2v_gemm_i8", epi->gelu) != P2V_OK) return P2V_E_ARG;
  if (kind == P2V_EPI_RESID && (!epi->s_mid || !epi->s_res || !epi->s_next || !epi->residual)) return fail(P2V_E_ARG, "RESID epilogue needs s_mid/s_res/s_next/residual");
  if (kind == P2V_EPI_EMBED && (!epi->s_next || !epi->pos_deq || epi->patches <= 0)) return fail(P2V_E_ARG, "EMBED epilogue needs s_next/pos_deq/patches");
  if (kind == P2V_EPI_RESID && out_codes) {      // the mid-code tap: 16-byte stores like `out`, int8-stored weights (packed int4: p2v_gemm_resid_tap)
    if ((uintptr_t)out_codes % 16 || (uintptr_t)out % 16) return fail(P2V_E_ARG, "p2v_gemm_i8: RESID out_codes and out must be 16-byte aligned");
    if (lin->packed4) return fail(P2V_E_UNSUPPORTED, "p2v_gemm_i8: the RESID mid-code tap takes int8-stored weights (packed4 = 0); p2v_gemm_resid_tap takes both");
  }
  if (kind != P2V_EPI_RESID && kind != P2V_EPI_HEAD) out_codes = nullptr;
  return run_gemm(kind, A, lda, M, K, N, *lin, *epi, out, ldo, out_codes, (hipStream_t)stream);
}

int p2v_gemm_resid_tap(const int8_t* A, int lda, int M, int K, int N, const p2v_linear* lin, const p2v_epilogue* epi, int8_t* out, int ldo,
                       int8_t* out_codes, void* stream) {
  if (!A || !lin || !epi || !out || !out_codes) return fail(P2V_E_ARG, "p2v_gemm_resid_tap: null argument");
  if (M <= 0 || N <= 0 || K <= 0 || K % GBK_PAD) return fail(P2V_E_SHAPE, "K=%d must be a positive multiple of %d", K, GBK_PAD);
  if (N % 16 || ldo % 16 || lda % 16) return fail(P2V_E_UNSUPPORTED, "p2v_gemm_resid_tap: N, lda and ldo must be multiples of 16");
  if (lda <= 0 || ldo < N) return fail(P2V_E_SHAPE, "p2v_gemm_resid_tap: lda=%d must be positive and ldo=%d must cover the %d outputs of a row", lda, ldo, N);
  if (!epi->s_mid || !epi->s_res || !epi->s_next || !epi->residual) return fail(P2V_E_ARG, "RESID epilogue needs s_mid/s_res/s_next/residual");
  if ((uintptr_t)out_codes % 16 || (uintptr_t)out % 16) return fail(P2V_E_ARG, "p2v_gemm_resid_tap: out_codes and out must be 16-byte aligned");
  if ((long long)M * ldo >= (1LL << 32)) return fail(P2V_E_SHAPE, "p2v_gemm_resid_tap: M * ldo = %lld passes the 32-bit offsets of the tapped stores", (long long)M * ldo);
  return run_gemm(P2V_EPI_RESID, A, lda, M, K, N, *lin, *epi, out, ldo, out_codes, (hipStream_t)stream);
}

int p2v_gemm_embed_tap(const int8_t* A, int lda, int M, int K, int N, const p2v_linear* lin, const p2v_epilogue* epi, int8_t* out, int ldo,
                       int8_t* pe_codes, int8_t* embed_codes, void* stream) {
  if (!A || !lin || !epi || !out || !pe_codes || !embed_codes) return fail(P2V_E_ARG, "p2v_gemm_embed_tap: null argument");
  if (M <= 0 || N <= 0 || K <= 0 || K % GBK_PAD) return fail(P2V_E_SHAPE, "K=%d must be a positive multiple of %d", K, GBK_PAD);
  if (N % 16 || ldo % 16 || lda % 16) return fail(P2V_E_UNSUPPORTED, "p2v_gemm_embed_tap: N, lda and ldo must be multiples of 16");
  if (lda <= 0 || ldo < N) return fail(P2V_E_SHAPE, "p2v_gemm_embed_tap: lda=%d must be positive and ldo=%d must cover the %d outputs of a row", lda, ldo, N);
  if (!epi->s_next || !epi->pos_deq || epi->patches <= 0) return fail(P2V_E_ARG, "EMBED epilogue needs s_next/pos_deq/patches");
  if ((uintptr_t)out % 16 || (uintptr_t)pe_codes % 16 || (uintptr_t)embed_codes % 16)
    return fail(P2V_E_ARG, "p2v_gemm_embed_tap: out, pe_codes and embed_codes must be 16-byte aligned");
  GemmArgs g = gemm_args(A, lda, M, lin->w_codes, K, N, *lin, *epi, out, ldo, pe_codes);
  g.out_codes2 = embed_codes;
  return launch_rc(p2v_launch_gemm(P2V_EPI_EMBED, g, (hipStream_t)stream), "gemm_i8");
}

size_t p2v_ln_prefold_bytes(int C) { return C > 0 ? (size_t)2 * round_up(C, 256) * sizeof(float) : 0; }

int p2v_ln_prefold(p2v_ln* ln, int C, float* buf, size_t buf_bytes) {
  if (!ln || !buf) return fail(P2V_E_ARG, "p2v_ln_prefold: null argument");
  ln->pre = kNoPre;
  if (C <= 0 || C % 4 || C > P2V_LN_MAX_C) return fail(P2V_E_SHAPE, "p2v_ln_prefold: C must be a positive multiple of 4 up to %d", P2V_LN_MAX_C);
  if (!ln_constants_present(*ln, false)) return fail(P2V_E_ARG, "p2v_ln_prefold: LayerNorm constants missing");      // (the fold does not read the mask)
  if (buf_bytes < p2v_ln_prefold_bytes(C)) return fail(P2V_E_WORKSPACE, "p2v_ln_prefold: buffer %zu < %zu bytes", buf_bytes, p2v_ln_prefold_bytes(C));
  OwnerDevice own(buf);
  if (!own.ok()) return fail(P2V_E_ARG, "p2v_ln_prefold: buf is not a device pointer");
  hipError_t e = hipDeviceSynchronize();                        // the caller's uploads may still be in flight
  p2v_ln_pre pre;
  if (e == hipSuccess) e = fold_one_ln(*ln, C, buf, &pre);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(P2V_E_LAUNCH, "p2v_ln_prefold: %s", hipGetErrorString(e));
  }
  ln->pre = pre;
  return P2V_OK;
}

size_t p2v_freeze_bytes(int N, int K, int layout) {
  if (N < 1 || K < 1 || K > (1 << 30) || layout < P2V_W_ROWS_I8 || layout > P2V_W_FRAG_P4) return 0;
  const size_t codes = ((size_t)N + 127) / 128 * 128 * (size_t)round_up(K, GBK_PAD);
  return layout == P2V_W_TILES_P4 || layout == P2V_W_FRAG_P4 ? codes / 2 : codes;
}

int p2v_freeze_weights(const float* w, long long ldw, int N, int K, const float* scale, int n_scale, int bits, int layout, void* out,
                       size_t out_bytes, void* stream) {
  if (!w || !scale || !out) return fail(P2V_E_ARG, "p2v_freeze_weights: null argument");
  if ((uintptr_t)w % 4 || (uintptr_t)scale % 4 || (uintptr_t)out % 16) return fail(P2V_E_ARG, "p2v_freeze_weights: w / scale must be 4-byte, out 16-byte aligned");
  if (N < 1 || K < 1 || K > (1 << 30) || ldw < K) return fail(P2V_E_SHAPE, "p2v_freeze_weights: N=%d K=%d ldw=%lld", N, K, ldw);
  if (n_scale != 1 && n_scale != N) return fail(P2V_E_SHAPE, "p2v_freeze_weights: %d scales for %d rows (1 or N)", n_scale, N);
  if (layout < P2V_W_ROWS_I8 || layout > P2V_W_FRAG_P4) return fail(P2V_E_SHAPE, "p2v_freeze_weights: unknown layout %d", layout);
  if (bits != 4 && bits != 8) return fail(P2V_E_BITS, "p2v_freeze_weights: %d-bit codes (4 or 8)", bits);
  if (bits == 8 && (layout == P2V_W_TILES_P4 || layout == P2V_W_FRAG_P4)) return fail(P2V_E_BITS, "p2v_freeze_weights: the packed layouts hold 4-bit codes");
  const size_t need = p2v_freeze_bytes(N, K, layout);
  if (out_bytes < need) return fail(P2V_E_WORKSPACE, "p2v_freeze_weights: out %zu < %zu bytes", out_bytes, need);
  if (need >= ((size_t)1 << 41)) return fail(P2V_E_SHAPE, "p2v_freeze_weights: %zu output bytes pass the grid of one launch", need);
  return launch_rc(p2v_launch_freeze_weights(w, ldw, N, K, scale, n_scale, bits, layout, out, (hipStream_t)stream), "freeze_weights");
}

// ---- patch-similarity entropy (p2vit_psaq.hip)
static int psaq_check(const char* who, int images, int groups, int heads, int tokens, int head_dim) {
  if (images < 1 || groups < 1 || heads < 1) return fail(P2V_E_SHAPE, "%s: images %d, groups %d, heads %d must be positive", who, images, groups, heads);
  if (tokens < 3 || tokens > 1025) return fail(P2V_E_SHAPE, "%s: %d tokens (2 ... 1024 patch rows behind the dropped first row)", who, tokens);
  if (head_dim < 4 || head_dim > 128 || head_dim % 4) return fail(P2V_E_SHAPE, "%s: head_dim %d (a multiple of 4 up to 128)", who, head_dim);
  const long long T = tokens - 1;
  if ((long long)images * groups >= (1LL << 31) / (T * ((T + 31) / 32)))
    return fail(P2V_E_SHAPE, "%s: %d x %d groups of %d tokens pass the grid of one launch", who, images, groups, tokens);
  return P2V_OK;
}

size_t p2v_psaq_workspace_bytes(int images, int groups, int heads, int tokens, int head_dim) {
  if (psaq_check("p2v_psaq_workspace_bytes", images, groups, heads, tokens, head_dim) != P2V_OK) return 0;
  return (size_t)p2v_psaq_layout(images, groups, tokens, head_dim).bytes;
}

int p2v_patch_similarity_entropy(const float* av, int images, int groups, int heads, int tokens, int head_dim, void* workspace,
                                 double* value_out, float* grad_out, void* stream) {
  const int rc = psaq_check("p2v_patch_similarity_entropy", images, groups, heads, tokens, head_dim);
  if (rc != P2V_OK) return rc;
  if (!av || !workspace || !value_out || !grad_out) return fail(P2V_E_ARG, "p2v_patch_similarity_entropy: null argument");
  if ((uintptr_t)av % 16 || (uintptr_t)grad_out % 16 || (uintptr_t)value_out % 8 || (uintptr_t)workspace % 256)
    return fail(P2V_E_ARG, "p2v_patch_similarity_entropy: av / grad_out must be 16-byte, value_out 8-byte, workspace 256-byte aligned");
  const PsaqArgs a = {av, images, groups, heads, tokens, head_dim};
  return launch_rc(p2v_launch_psaq(a, workspace, value_out, grad_out, (hipStream_t)stream), "patch_similarity_entropy");
}

// ---- Hutchinson trace bookkeeping (p2vit_hessian.hip)
static int hs_check_n(const char* who, int n_segs) {
  if (n_segs < 1 || n_segs > 65536) return fail(P2V_E_ARG, "%s: n_segs = %d (1 ... 65536)", who, n_segs);
  return P2V_OK;
}
static int hs_check_segs(const char* who, const p2v_seg* segs, int n_segs) {
  if (const int rc = hs_check_n(who, n_segs)) return rc;
  if (!segs) return fail(P2V_E_ARG, "%s: null argument", who);
  for (int s = 0; s < n_segs; ++s) {
    if (!segs[s].ptr || (uintptr_t)segs[s].ptr % 4) return fail(P2V_E_ARG, "%s: segment %d: null or misaligned pointer", who, s);
    if (segs[s].n < 1 || segs[s].n > 0x7fffffffLL) return fail(P2V_E_ARG, "%s: segment %d: n = %lld (1 ... 2^31 - 1)", who, s, segs[s].n);
  }
  return P2V_OK;
}
static int hs_check_segs2(const char* who, const p2v_seg2* segs, int n_segs) {
  if (const int rc = hs_check_n(who, n_segs)) return rc;
  if (!segs) return fail(P2V_E_ARG, "%s: null argument", who);
  for (int s = 0; s < n_segs; ++s) {
    if (!segs[s].a || !segs[s].b || (uintptr_t)segs[s].a % 4 || (uintptr_t)segs[s].b % 4)
      return fail(P2V_E_ARG, "%s: segment %d: null or misaligned pointer", who, s);
    if (segs[s].n < 1 || segs[s].n > 0x7fffffffLL) return fail(P2V_E_ARG, "%s: segment %d: n = %lld (1 ... 2^31 - 1)", who, s, segs[s].n);
  }
  return P2V_OK;
}

int p2v_rademacher_fill(const p2v_seg* segs, int n_segs, uint64_t seed, uint64_t probe, void* stream) {
  if (const int rc = hs_check_segs("p2v_rademacher_fill", segs, n_segs)) return rc;
  return launch_rc(p2v_launch_rademacher_fill(segs, n_segs, seed, probe, (hipStream_t)stream), "rademacher_fill");
}

size_t p2v_group_dot_workspace_bytes(const p2v_seg2* segs, int n_segs) {
  if (hs_check_segs2("p2v_group_dot_workspace_bytes", segs, n_segs) != P2V_OK) return 0;
  return (size_t)p2v_hs_dot_chunks(segs, n_segs) * sizeof(double);
}

static int hs_check_dot(const char* who, const p2v_seg2* segs, int n_segs, const void* out, const void* ws, size_t ws_bytes) {
  if (const int rc = hs_check_segs2(who, segs, n_segs)) return rc;
  if (!out || !ws) return fail(P2V_E_ARG, "%s: null argument", who);
  if ((uintptr_t)out % 8 || (uintptr_t)ws % 8) return fail(P2V_E_ARG, "%s: out / record and ws must be 8-byte aligned", who);
  const size_t need = (size_t)p2v_hs_dot_chunks(segs, n_segs) * sizeof(double);
  if (ws_bytes < need) return fail(P2V_E_WORKSPACE, "%s: workspace %zu < %zu bytes", who, ws_bytes, need);
  return P2V_OK;
}

int p2v_group_dot(const p2v_seg2* segs, int n_segs, double* out, void* ws, size_t ws_bytes, void* stream) {
  if (const int rc = hs_check_dot("p2v_group_dot", segs, n_segs, out, ws, ws_bytes)) return rc;
  return launch_rc(p2v_launch_group_dot(segs, n_segs, out, static_cast<double*>(ws), nullptr, 0, 0.0, (hipStream_t)stream), "group_dot");
}

size_t p2v_hutchinson_state_bytes(int n_segs) { return n_segs < 1 || n_segs > 65536 ? 0 : p2v_hs_state_bytes(n_segs); }

int p2v_hutchinson_init(void* state, size_t state_bytes, int n_segs, void* stream) {
  if (const int rc = hs_check_n("p2v_hutchinson_init", n_segs)) return rc;
  if (!state || (uintptr_t)state % 8) return fail(P2V_E_ARG, "p2v_hutchinson_init: null or misaligned state");
  if (state_bytes < p2v_hs_state_bytes(n_segs)) return fail(P2V_E_WORKSPACE, "p2v_hutchinson_init: state %zu < %zu bytes", state_bytes, p2v_hs_state_bytes(n_segs));
  return launch_rc(p2v_launch_hutchinson_init(state, n_segs, (hipStream_t)stream), "hutchinson_init");
}

int p2v_hutchinson_step(const p2v_seg2* segs, int n_segs, int probe, int max_iter, double tol, double* record, void* state,
                        size_t state_bytes, void* ws, size_t ws_bytes, void* stream) {
  if (const int rc = hs_check_dot("p2v_hutchinson_step", segs, n_segs, record, ws, ws_bytes)) return rc;
  if (!state || (uintptr_t)state % 8) return fail(P2V_E_ARG, "p2v_hutchinson_step: null or misaligned state");
  if (max_iter < 1 || probe < 0 || probe >= max_iter) return fail(P2V_E_ARG, "p2v_hutchinson_step: probe %d outside 0 ... max_iter - 1 = %d", probe, max_iter - 1);
  if (tol != tol) return fail(P2V_E_ARG, "p2v_hutchinson_step: tol is not a number");
  if (state_bytes < p2v_hs_state_bytes(n_segs)) return fail(P2V_E_WORKSPACE, "p2v_hutchinson_step: state %zu < %zu bytes", state_bytes, p2v_hs_state_bytes(n_segs));
  return launch_rc(p2v_launch_group_dot(segs, n_segs, record + (size_t)probe * n_segs, static_cast<double*>(ws), state, probe, tol, (hipStream_t)stream),
                   "hutchinson_step");
}

size_t p2v_resid_prefold_bytes(int N) { return N > 0 ? resid_tab_floats(N) * sizeof(float) : 0; }

int p2v_resid_prefold(const p2v_linear* lin, const p2v_epilogue* epi, int N, float* tab, size_t tab_bytes, int* usable, void* stream) {
  if (!lin || !epi || !tab || !usable) return fail(P2V_E_ARG, "p2v_resid_prefold: null argument");
  *usable = 0;
  if (N <= 0) return fail(P2V_E_SHAPE, "p2v_resid_prefold: N must be positive");
  if (!lin->colscale || !lin->bias || !epi->s_mid || !epi->s_res || !epi->s_next) return fail(P2V_E_ARG, "p2v_resid_prefold: needs colscale / bias / s_mid / s_res / s_next");
  if (tab_bytes < p2v_resid_prefold_bytes(N)) return fail(P2V_E_WORKSPACE, "p2v_resid_prefold: table %zu < %zu bytes", tab_bytes, p2v_resid_prefold_bytes(N));
  if (const int cap = refuse_capture("p2v_resid_prefold", "allocates its flags and reads them back to the host", stream)) return cap;
  OwnerDevice dev(tab);
  if (!dev.ok()) return fail(P2V_E_ARG, "p2v_resid_prefold: tab is not a device pointer");
  return resid_prefold_impl(*lin, *epi, N, tab, usable, (hipStream_t)stream);
}

int p2v_int_layernorm(const int8_t* x, long long row_stride, int rows, int C, const p2v_ln* ln, int8_t* out, long long out_stride,
                      void* stream) {
  if (!x || !ln || !out) return fail(P2V_E_ARG, "p2v_int_layernorm: null argument");
  if (C % 4 || row_stride % 4 || out_stride % 4) return fail(P2V_E_UNSUPPORTED, "C and strides must be multiples of 4");
  if (rows <= 0) return fail(P2V_E_SHAPE, "rows must be positive");
  if (C <= 0 || row_stride < 0 || out_stride < C) return fail(P2V_E_SHAPE, "p2v_int_layernorm: C=%d must be positive, row_stride non-negative, out_stride >= C", C);
  if (C > P2V_LN_MAX_C) return fail(P2V_E_SHAPE, "p2v_int_layernorm: C=%d, the LayerNorm kernels cover up to %d channels", C, P2V_LN_MAX_C);
  // rows beyond 2048 channels (new with the row-per-workgroup kernel) are taken only as whole rows: a row_stride inside the row would make
  // the input rows overlap.  Up to 2048 channels the entry point keeps what it accepted before.
  if (C > 2048 && row_stride < C)
    return fail(P2V_E_SHAPE, "p2v_int_layernorm: C=%d beyond 2048 channels needs row_stride >= C (got %lld)", C, row_stride);
  LnArgs a{x, row_stride, rows, C, *ln, out, out_stride};
  a.pre = ln->pre;                       // optional: constants folded ahead of the launch (p2v_ln_prefold)
  return launch_rc(p2v_launch_layernorm(a, (hipStream_t)stream), "int_layernorm");
}

int p2v_int_layernorm_tap(const int8_t* x, long long row_stride, int rows, int C, const p2v_ln* ln, int8_t* out, long long out_stride,
                          float* tap_out, void* stream) {
  if (!x || !ln || !out || !tap_out) return fail(P2V_E_ARG, "p2v_int_layernorm_tap: null argument");
  if (C % 4 || row_stride % 4 || out_stride % 4) return fail(P2V_E_UNSUPPORTED, "C and strides must be multiples of 4");
  if (rows <= 0) return fail(P2V_E_SHAPE, "rows must be positive");
  if (C <= 0 || row_stride < 0 || out_stride < C) return fail(P2V_E_SHAPE, "p2v_int_layernorm_tap: C=%d must be positive, row_stride non-negative, out_stride >= C", C);
  if (C > 2048) return fail(P2V_E_UNSUPPORTED, "p2v_int_layernorm_tap: C=%d, the value tap covers rows of up to 2048 channels", C);
  if ((uintptr_t)tap_out % 16) return fail(P2V_E_ARG, "p2v_int_layernorm_tap: tap_out must be 16-byte aligned");
  LnArgs a{x, row_stride, rows, C, *ln, out, out_stride};
  a.pre = ln->pre;
  a.tap_out = tap_out;
  return launch_rc(p2v_launch_layernorm(a, (hipStream_t)stream), "int_layernorm");
}

int p2v_ln_gemm_i8(int kind, const int8_t* x, long long row_stride, int M, int C, const p2v_ln* ln, int N, const p2v_linear* lin,
                   const p2v_epilogue* epi, int8_t* out, int ldo, int8_t* ln_out, void* stream) {
  if (!x || !ln || !lin || !epi || !out) return fail(P2V_E_ARG, "p2v_ln_gemm_i8: null argument");
  if (kind != P2V_EPI_REQUANT && kind != P2V_EPI_GELU) return fail(P2V_E_ARG, "p2v_ln_gemm_i8: epilogue %d (REQUANT and GELU are fused)", kind);
  if (M <= 0 || C <= 0 || N <= 0) return fail(P2V_E_SHAPE, "p2v_ln_gemm_i8: bad shape");
  if (C % 4 || row_stride % 4 || N % 16 || ldo != N) return fail(P2V_E_UNSUPPORTED, "p2v_ln_gemm_i8: C, row_stride multiples of 4; N multiple of 16; ldo == N");
  if (row_stride < 0) return fail(P2V_E_SHAPE, "p2v_ln_gemm_i8: negative row_stride");
  if (kind == P2V_EPI_REQUANT && check_requant_scale("p2v_ln_gemm_i8", epi->inv_s_out) != P2V_OK) return P2V_E_UNSUPPORTED;
  if (kind == P2V_EPI_GELU && check_gelu_tab("p2v_ln_gemm_i8", epi->gelu) != P2V_OK) return P2V_E_ARG;
  read_env_once();
  LnArgs a{x, row_stride, M, C, *ln, ln_out, C};
  a.pre = ln->pre;
  return run_ln_gemm(kind, a, *lin, *epi, N, out, (hipStream_t)stream);
}

int p2v_ln_gemm_fusable(int kind, int C, int N, int cells) {
  read_env_once();
  return (C > 0 && N > 0 && cells >= 0 && cells <= 4096 && p2v_ln_gemm_supported(kind, C, N, cells)) ? 1 : 0;
}

// both attention entry points; query_rows 0 (below min_rows for the entry point that takes a count): every row
// the pitched tap planes of the two _taps entry points: checked only when one is given
static int check_tap_planes(const char* who, int row, int pitch, std::initializer_list<const void*> planes) {
  bool any = false;
  for (const void* q : planes) any = any || q;
  if (!any) return P2V_OK;
  if (pitch < row || pitch % 16) return fail(P2V_E_ARG, "%s: pitch %d must be a multiple of 16 and at least the row length %d", who, pitch, row);
  for (const void* q : planes)
    if ((uintptr_t)q % 16) return fail(P2V_E_ARG, "%s: the tap planes must be 16-byte aligned", who);
  return P2V_OK;
}

static int lis_attention(const char* who, int bits, const int8_t* qkv, int batch, int tokens, int heads, int head_dim, const p2v_attn* at, int min_rows,
                         int query_rows, int8_t* out, int8_t* probs_k, void* stream, int8_t* score_codes = nullptr, int8_t* probs_kp = nullptr,
                         int pitch = 0) {
  if (!qkv || !at || !out) return fail(P2V_E_ARG, "%s: null argument", who);
  if (batch <= 0 || tokens <= 0 || heads <= 0) return fail(P2V_E_SHAPE, "bad attention shape");
  if (query_rows < min_rows || query_rows > tokens) return fail(P2V_E_SHAPE, "%s: query_rows %d outside 1 .. %d", who, query_rows, tokens);
  const int rc = check_attn(who, *at, bits);
  if (rc != P2V_OK) return rc;
  const int rp = check_tap_planes(who, tokens, pitch, {score_codes, probs_kp});
  if (rp != P2V_OK) return rp;
  AttnArgs a{{qkv, batch, tokens, heads, *at, out, probs_k}};
  a.nq = query_rows;
  a.klim = 1 << bits;
  a.score_codes = score_codes; a.probs_kp = probs_kp; a.pitch = pitch;
  return launch_rc(p2v_launch_attention(a, head_dim, (hipStream_t)stream), "lis_attention");
}

int p2v_lis_attention_taps(const int8_t* qkv, int batch, int tokens, int heads, int head_dim, const p2v_attn* at, int8_t* out,
                           int8_t* score_codes, int8_t* probs_k, int pitch, void* stream) {
  return lis_attention("p2v_lis_attention_taps", 4, qkv, batch, tokens, heads, head_dim, at, 0, 0, out, nullptr, stream, score_codes, probs_k, pitch);
}
int p2v_lis_attention_taps_bits(const int8_t* qkv, int batch, int tokens, int heads, int head_dim, const p2v_attn* at, int softmax_bits,
                                int8_t* out, int8_t* score_codes, int8_t* probs_k, int pitch, void* stream) {
  return lis_attention("p2v_lis_attention_taps_bits", softmax_bits, qkv, batch, tokens, heads, head_dim, at, 0, 0, out, nullptr, stream, score_codes,
                       probs_k, pitch);
}

int p2v_lis_attention(const int8_t* qkv, int batch, int tokens, int heads, int head_dim, const p2v_attn* at, int8_t* out,
                      int8_t* probs_k, void* stream) {
  return lis_attention("p2v_lis_attention", 4, qkv, batch, tokens, heads, head_dim, at, 0, 0, out, probs_k, stream);
}
int p2v_lis_attention_bits(const int8_t* qkv, int batch, int tokens, int heads, int head_dim, const p2v_attn* at, int softmax_bits,
                           int8_t* out, int8_t* probs_k, void* stream) {
  return lis_attention("p2v_lis_attention_bits", softmax_bits, qkv, batch, tokens, heads, head_dim, at, 0, 0, out, probs_k, stream);
}

int p2v_lis_attention_rows(const int8_t* qkv, int batch, int tokens, int heads, int head_dim, const p2v_attn* at, int query_rows,
                           int8_t* out, void* stream) {
  return lis_attention("p2v_lis_attention_rows", 4, qkv, batch, tokens, heads, head_dim, at, 1, query_rows, out, nullptr, stream);
}
int p2v_lis_attention_rows_bits(const int8_t* qkv, int batch, int tokens, int heads, int head_dim, const p2v_attn* at, int softmax_bits,
                                int query_rows, int8_t* out, void* stream) {
  return lis_attention("p2v_lis_attention_rows_bits", softmax_bits, qkv, batch, tokens, heads, head_dim, at, 1, query_rows, out, nullptr, stream);
}

// ---- float LayerNorm / table softmax (Config(ptf=False) / Config(lis=False)) -------------------------------------------------------------
static int check_float_ln(const char* who, const p2v_float_ln& l) {
  if (!l.gamma || !l.beta || !l.g) return fail(P2V_E_ARG, "%s: float LayerNorm constants missing", who);
  if ((uintptr_t)l.gamma % 16 || (uintptr_t)l.beta % 16 || (uintptr_t)l.g % 16) return fail(P2V_E_ARG, "%s: gamma / beta / g must be 16-byte aligned", who);
  if (!is_pot(l.s_in) || l.s_in < 0x1p-40f || l.s_in > 0x1p40f) return fail(P2V_E_UNSUPPORTED, "%s: input scale %g must be a power of two", who, l.s_in);
  if (!(l.eps > 0.f)) return fail(P2V_E_ARG, "%s: eps must be positive", who);
  return P2V_OK;
}
static int check_softmax_attn(const char* who, const p2v_softmax_attn& at) {
  if (!at.table || (uintptr_t)at.table % 4) return fail(P2V_E_ARG, "%s: null or misaligned softmax table", who);
  if (!is_pot(at.s_qkv_sq * at.inv_s_attn)) return fail(P2V_E_UNSUPPORTED, "%s: s_qkv_sq * inv_s_attn must be a power of two", who);
  if (!(at.qk_scale > 0.f)) return fail(P2V_E_ARG, "%s: qk_scale must be positive", who);
  if (!is_pot(at.av_mul) || at.av_mul > 0x1p15f || at.av_mul < 0x1p-40f)
    return fail(P2V_E_UNSUPPORTED, "%s: av_mul %g must be a power of two in [2^-40, 2^15]", who, at.av_mul);
  return P2V_OK;
}
static int check_softmax_shape(const char* who, int head_dim, int tokens) {
  if (head_dim != 32 && head_dim != 64) return fail(P2V_E_UNSUPPORTED, "%s: head_dim %d (the table-softmax attention covers 32 and 64)", who, head_dim);
  if (tokens > P2V_MAX_TOKENS) return fail(P2V_E_UNSUPPORTED, "%s: %d tokens per image, the table-softmax attention covers up to %d", who, tokens, P2V_MAX_TOKENS);
  return P2V_OK;
}

int p2v_float_layernorm(const int8_t* x, long long row_stride, int rows, int C, const p2v_float_ln* ln, int8_t* out, long long out_stride,
                        float* tap_out, void* stream) {
  if (!x || !ln || !out) return fail(P2V_E_ARG, "p2v_float_layernorm: null argument");
  if (C % 4 || row_stride % 4 || out_stride % 4) return fail(P2V_E_UNSUPPORTED, "C and strides must be multiples of 4");
  if (rows <= 0) return fail(P2V_E_SHAPE, "rows must be positive");
  if (C < 16 || C > P2V_FLOAT_LN_MAX_C) return fail(P2V_E_SHAPE, "p2v_float_layernorm: C=%d, the kernels cover 16 .. %d channels", C, P2V_FLOAT_LN_MAX_C);
  if (row_stride < 0 || out_stride < C) return fail(P2V_E_SHAPE, "p2v_float_layernorm: row_stride non-negative, out_stride >= C");
  // as p2v_int_layernorm: rows beyond 2048 channels (the row-per-workgroup kernel) are taken only as whole rows.  Up to 2048 channels the
  // entry point keeps what it accepted before.
  if (C > 2048 && row_stride < C)
    return fail(P2V_E_SHAPE, "p2v_float_layernorm: C=%d beyond 2048 channels needs row_stride >= C (got %lld)", C, row_stride);
  if ((uintptr_t)x % 4 || (uintptr_t)out % 4 || (uintptr_t)tap_out % 16) return fail(P2V_E_ARG, "p2v_float_layernorm: x / out 4-byte, tap_out 16-byte aligned");
  if (const int rc = check_float_ln("p2v_float_layernorm", *ln)) return rc;
  const FloatLnArgs a{x, row_stride, rows, C, (double)ln->s_in, (double)ln->eps, ln->gamma, ln->beta, ln->g, out, out_stride, tap_out};
  return launch_rc(p2v_launch_float_layernorm(a, (hipStream_t)stream), "float_layernorm");
}

int p2v_float_layernorm_max_channels(void) { return P2V_FLOAT_LN_MAX_C; }

int p2v_softmax_attention_taps(const int8_t* qkv, int batch, int tokens, int heads, int head_dim, const p2v_softmax_attn* at, int8_t* out,
                               int8_t* score_codes, int pitch, void* stream) {
  const char* who = "p2v_softmax_attention";
  if (!qkv || !at || !out) return fail(P2V_E_ARG, "%s: null argument", who);
  if (batch <= 0 || tokens <= 0 || heads <= 0) return fail(P2V_E_SHAPE, "bad attention shape");
  int rc = check_softmax_shape(who, head_dim, tokens);
  if (rc == P2V_OK) rc = check_softmax_attn(who, *at);
  if (rc == P2V_OK) rc = check_tap_planes(who, tokens, pitch, {score_codes});
  if (rc != P2V_OK) return rc;
  if ((uintptr_t)qkv % 16 || (uintptr_t)out % 4) return fail(P2V_E_ARG, "%s: qkv 16-byte, out 4-byte aligned", who);
  read_env_once();
  const SmAttnArgs a{qkv, batch, tokens, heads, at->s_qkv_sq, at->qk_scale, at->inv_s_attn, at->av_mul, at->table, out, score_codes, pitch, 0};
  return launch_rc(p2v_launch_softmax_attention(a, head_dim, (hipStream_t)stream), who);
}

int p2v_softmax_attention(const int8_t* qkv, int batch, int tokens, int heads, int head_dim, const p2v_softmax_attn* at, int8_t* out,
                          void* stream) {
  return p2v_softmax_attention_taps(qkv, batch, tokens, heads, head_dim, at, out, nullptr, 0, stream);
}

int p2v_plan_set_float_ops(p2v_plan* plan, int float_norm, int float_softmax) {
  if (!plan) return fail(P2V_E_ARG, "p2v_plan_set_float_ops: null plan");
  if (float_softmax)
    if (const int rc = check_softmax_shape("p2v_plan_set_float_ops", plan->d.embed_dim / plan->d.num_heads, plan->tokens)) return rc;
  plan->float_norm = float_norm != 0;
  plan->float_softmax = float_softmax != 0;
  return P2V_OK;
}

int p2v_plan_set_softmax_bits(p2v_plan* plan, int block, int bits) {
  const char* who = "p2v_plan_set_softmax_bits";
  if (!plan) return fail(P2V_E_ARG, "%s: null plan", who);
  if (block < 0 || block >= plan->d.depth) return fail(P2V_E_ARG, "%s: block %d out of range", who, block);
  if (plan->float_softmax) return fail(P2V_E_UNSUPPORTED, "%s: the plan's softmax is the table one, it has no width", who);
  if (const int rc = check_softmax_bits(who, bits)) return rc;
  if (plan->block_set[block] && plan->blocks[block].attn.av_mul > av_mul_max(bits))
    return fail(P2V_E_UNSUPPORTED, "%s: av_mul %g of block %d is above 2^7, the range of a 3-bit softmax", who, plan->blocks[block].attn.av_mul, block);
  plan->softmax_bits[block] = (char)bits;
  return P2V_OK;
}

int p2v_plan_set_float_block(p2v_plan* plan, int block, const p2v_float_block* blk) {
  if (!plan || !blk) return fail(P2V_E_ARG, "p2v_plan_set_float_block: null argument");
  if (block < 0 || block >= plan->d.depth) return fail(P2V_E_ARG, "block %d out of range", block);
  if (plan->float_norm)
    for (int i = 0; i < 6; ++i)
      if (const int rc = check_float_ln("p2v_plan_set_float_block", block_ln(*blk, i))) return rc;
  if (plan->float_softmax) {
    if (!blk->softmax_table || (uintptr_t)blk->softmax_table % 4) return fail(P2V_E_ARG, "p2v_plan_set_float_block: null or misaligned softmax table");
    // den >= table[0] > 0 and the three 7-bit digits: read back once (synchronises, like the LayerNorm fold of p2v_plan_set_block)
    OwnerDevice own(blk->softmax_table);
    uint32_t tab[256];
    if (!own.ok() || hipDeviceSynchronize() != hipSuccess || hipMemcpy(tab, blk->softmax_table, sizeof tab, hipMemcpyDeviceToHost) != hipSuccess) {
      (void)hipGetLastError();
      return fail(P2V_E_ARG, "p2v_plan_set_float_block: cannot read the softmax table (a device pointer?)");
    }
    if (tab[0] == 0) return fail(P2V_E_ARG, "p2v_plan_set_float_block: softmax table entry 0 must be positive");
    for (int d = 0; d < 256; ++d)
      if (tab[d] >= (1u << 21)) return fail(P2V_E_ARG, "p2v_plan_set_float_block: softmax table entry %d = %u, must be below 2^21", d, tab[d]);
  }
  plan->fblocks[block] = *blk;
  plan->fblock_set[block] = 1;
  return P2V_OK;
}

int p2v_plan_set_float_head(p2v_plan* plan, const p2v_float_ln* final_ln) {
  if (!plan || !final_ln) return fail(P2V_E_ARG, "p2v_plan_set_float_head: null argument");
  if (const int rc = check_float_ln("p2v_plan_set_float_head", *final_ln)) return rc;
  plan->final_fln = *final_ln;
  plan->fhead_set = true;
  return P2V_OK;
}

int p2v_patch_merge_gather(const int8_t* x, int batch, int H, int W, int C, int8_t* out, void* stream) {
  if (!x || !out) return fail(P2V_E_ARG, "p2v_patch_merge_gather: null argument");
  if (batch <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return fail(P2V_E_SHAPE, "patch merge: H and W must be positive and even");
  if (C <= 0 || C % 16) return fail(P2V_E_UNSUPPORTED, "patch merge: C must be a multiple of 16");
  return launch_rc(p2v_launch_patch_merge_gather(x, batch, H, W, C, out, (hipStream_t)stream), "patch_merge_gather");
}

int p2v_avgpool_quant(const int8_t* x, int batch, int tokens, int C, float s_in, float inv_s_out, int8_t* out, void* stream) {
  if (!x || !out) return fail(P2V_E_ARG, "p2v_avgpool_quant: null argument");
  if (batch <= 0 || tokens <= 0 || tokens > 8192) return fail(P2V_E_SHAPE, "avgpool: bad shape");
  if (C <= 0 || C % 4) return fail(P2V_E_UNSUPPORTED, "avgpool: C must be a multiple of 4");
  return launch_rc(p2v_launch_avgpool_quant(x, batch, tokens, C, s_in, inv_s_out, out, (hipStream_t)stream), "avgpool_quant");
}

static int window_attention(const char* who, int bits, const int8_t* qkv, int batch, int tokens_per_image, int heads, int head_dim, const p2v_winattn* wa,
                            int8_t* out, int8_t* probs_k, void* stream, int8_t* attn1_codes, int8_t* qact2_codes, int8_t* probs_kp, int pitch) {
  if (!qkv || !wa || !out || !wa->table_codes || !wa->win_index) return fail(P2V_E_ARG, "p2v_window_attention: null argument");
  if (batch <= 0 || tokens_per_image <= 0 || heads <= 0) return fail(P2V_E_SHAPE, "bad window attention shape");
  if (head_dim != 32) return fail(P2V_E_UNSUPPORTED, "window attention: head_dim must be 32");
  if (const int rb = check_softmax_bits(who, bits)) return rb;
  if (wa->ws < 1 || wa->ws > 12 || wa->n_windows < 1 || wa->ws * wa->ws * wa->n_windows > tokens_per_image)
    return fail(P2V_E_SHAPE, "window attention: window size must be 1..12 and windows must fit the token count");
  {
    const int rc = check_lis_consts("p2v_window_attention", wa->x0_int, wa->b_int, wa->c_int);
    if (rc != P2V_OK) return rc;
  }
  const float pots[5] = {wa->s_q1, wa->s_attn, wa->s_table, wa->s_q2, wa->s_q3};
  for (float s : pots) {
    int ex;
    if (!(s > 0.f) || frexpf(s, &ex) != 0.5f) return fail(P2V_E_UNSUPPORTED, "window attention: activation scales must be powers of two");
  }
  if (wa->qkv_stride % 16 || wa->out_stride % 4 || (wa->qkv_stride && wa->qkv_stride < 3 * heads * head_dim) ||
      (wa->out_stride && wa->out_stride < heads * head_dim))
    return fail(P2V_E_SHAPE, "window attention: row strides must cover a row and be 16 / 4 byte aligned");
  if (wa->s_q2 > 1.0f) return fail(P2V_E_UNSUPPORTED, "window attention: qact2 scale above 1 (the -100 mask would not be an integer)");
  if (wa->s_q1 / wa->s_q3 > av_mul_max(bits) || wa->s_q1 / wa->s_q3 < 0x1p-40f)
    return fail(P2V_E_UNSUPPORTED, "window attention: qact1 scale / qact3 scale must lie in [2^-40, 2^%d] at softmax_bits %d", bits == 3 ? 7 : 15, bits);
  const int rp = check_tap_planes(who, wa->ws * wa->ws, pitch, {attn1_codes, qact2_codes, probs_kp});
  if (rp != P2V_OK) return rp;
  WinAttnArgs a{{qkv, batch, tokens_per_image, heads, *wa, out, probs_k, 1 << bits}};
  a.attn1_codes = attn1_codes; a.qact2_codes = qact2_codes; a.probs_kp = probs_kp; a.pitch = pitch;
  return launch_rc(p2v_launch_window_attention(a, (hipStream_t)stream), "window_attention");
}

int p2v_window_attention(const int8_t* qkv, int batch, int tokens_per_image, int heads, int head_dim, const p2v_winattn* wa,
                         int8_t* out, int8_t* probs_k, void* stream) {
  return window_attention("p2v_window_attention", 4, qkv, batch, tokens_per_image, heads, head_dim, wa, out, probs_k, stream, nullptr, nullptr, nullptr, 0);
}
int p2v_window_attention_bits(const int8_t* qkv, int batch, int tokens_per_image, int heads, int head_dim, const p2v_winattn* wa,
                              int softmax_bits, int8_t* out, int8_t* probs_k, void* stream) {
  return window_attention("p2v_window_attention_bits", softmax_bits, qkv, batch, tokens_per_image, heads, head_dim, wa, out, probs_k, stream, nullptr,
                          nullptr, nullptr, 0);
}

int p2v_window_attention_taps(const int8_t* qkv, int batch, int tokens_per_image, int heads, int head_dim, const p2v_winattn* wa,
                              int8_t* out, int8_t* attn1_codes, int8_t* qact2_codes, int8_t* probs_k, int pitch, void* stream) {
  return window_attention("p2v_window_attention_taps", 4, qkv, batch, tokens_per_image, heads, head_dim, wa, out, nullptr, stream, attn1_codes,
                          qact2_codes, probs_k, pitch);
}
int p2v_window_attention_taps_bits(const int8_t* qkv, int batch, int tokens_per_image, int heads, int head_dim, const p2v_winattn* wa,
                                   int softmax_bits, int8_t* out, int8_t* attn1_codes, int8_t* qact2_codes, int8_t* probs_k, int pitch,
                                   void* stream) {
  return window_attention("p2v_window_attention_taps_bits", softmax_bits, qkv, batch, tokens_per_image, heads, head_dim, wa, out, nullptr, stream,
                          attn1_codes, qact2_codes, probs_k, pitch);
}

// Config(lis=False) of a Swin plan: the table softmax behind the qact2 codes.  Every refusal comes before the launch
int p2v_window_softmax_attention(const int8_t* qkv, int batch, int tokens_per_image, int heads, int head_dim, const p2v_winattn* wa,
                                 const uint32_t* table, int8_t* out, void* stream) {
  const char* who = "p2v_window_softmax_attention";
  if (!qkv || !wa || !table || !out || !wa->table_codes || !wa->win_index) return fail(P2V_E_ARG, "%s: null argument", who);
  if ((uintptr_t)qkv % 16 || (uintptr_t)out % 4 || (uintptr_t)table % 4 || (uintptr_t)wa->win_index % 4)
    return fail(P2V_E_ARG, "%s: qkv 16-byte, out / table / win_index 4-byte aligned", who);
  if (batch <= 0 || tokens_per_image <= 0 || heads <= 0) return fail(P2V_E_SHAPE, "%s: bad shape", who);
  if (head_dim != 32) return fail(P2V_E_UNSUPPORTED, "%s: head_dim must be 32", who);
  if (wa->ws < 1 || wa->ws > 12 || wa->n_windows < 1 || wa->ws * wa->ws * wa->n_windows > tokens_per_image)
    return fail(P2V_E_SHAPE, "%s: window size must be 1..12 and windows must fit the token count", who);
  const float pots[5] = {wa->s_q1, wa->s_attn, wa->s_table, wa->s_q2, wa->s_q3};
  for (float s : pots)
    if (!is_pot(s)) return fail(P2V_E_UNSUPPORTED, "%s: activation scales must be powers of two", who);
  if (wa->qkv_stride % 16 || wa->out_stride % 4 || (wa->qkv_stride && wa->qkv_stride < 3 * heads * head_dim) ||
      (wa->out_stride && wa->out_stride < heads * head_dim))
    return fail(P2V_E_SHAPE, "%s: row strides must cover a row and be 16 / 4 byte aligned", who);
  // a masked key counts as exactly zero: 100 / s_q2 > 255 codes below every key of the region, and exp(-(100 - 255 s_q2)) 2^21 rounds to 0
  if (wa->s_q2 > 0x1p-2f) return fail(P2V_E_UNSUPPORTED, "%s: qact2 scale %g above 2^-2 (a masked key would not round to zero)", who, wa->s_q2);
  const float av_mul = wa->s_q1 / wa->s_q3;
  if (!is_pot(av_mul) || av_mul > 0x1p15f || av_mul < 0x1p-40f)
    return fail(P2V_E_UNSUPPORTED, "%s: qact1 scale / qact3 scale = %g must be a power of two in [2^-40, 2^15]", who, av_mul);
  const WinSmArgs a{qkv, batch, tokens_per_image, heads, *wa, table, out};
  return launch_rc(p2v_launch_window_softmax_attention(a, (hipStream_t)stream), who);
}

// the layer output fmaf(acc, colscale, bias) as dense fp32 (P2V_OP_GEMM_F32): what a QLinear / QConv2d hook sees.  The public p2v_gemm_i8
// goes on refusing the internal epilogue kind.
static int gemm_f32_op(const p2v_op& o, void* stream) {
  if (!o.in || !o.out || !o.lin.w_codes || !o.lin.colscale || !o.lin.bias) return fail(P2V_E_ARG, "P2V_OP_GEMM_F32: null argument");
  if (o.M <= 0 || o.N <= 0 || o.K <= 0 || o.K % GBK_PAD) return fail(P2V_E_SHAPE, "P2V_OP_GEMM_F32: K=%d must be a positive multiple of %d", o.K, GBK_PAD);
  if (o.lda <= 0 || o.lda % 16) return fail(P2V_E_UNSUPPORTED, "P2V_OP_GEMM_F32: lda must be a positive multiple of 16");
  if (o.ldo < o.N || (o.ldo != o.N && o.ldo % 4)) return fail(P2V_E_SHAPE, "P2V_OP_GEMM_F32: ldo=%d must be N=%d, or a multiple of 4 beyond it", o.ldo, o.N);
  if ((uintptr_t)o.in % 16 || (uintptr_t)o.out % 16) return fail(P2V_E_ARG, "P2V_OP_GEMM_F32: in and out must be 16-byte aligned");
  return run_gemm(P2V_EPI_F32, (const int8_t*)o.in, o.lda, o.M, o.K, o.N, o.lin, p2v_epilogue{}, o.out, o.ldo, nullptr, (hipStream_t)stream);
}
static int cos_check(const p2v_cos_layer* layers, int n_layers, int n, const char* what);
static p2v_cos_layer cos_op_layer(const p2v_op& o) {
  const long long sample = (long long)(((unsigned long long)(unsigned)o.i3 << 32) | (unsigned)o.i2);
  const size_t esz = o.i1 == P2V_COS_F32 ? 4 : 1;
  const char* a = reinterpret_cast<const char*>(o.in);
  return p2v_cos_layer{a, a ? a + (size_t)(o.i0 > 0 ? o.i0 : 0) * (size_t)(sample > 0 ? sample : 0) * esz : nullptr, o.lin.colscale, sample, o.lda, o.M, o.N, o.i1};
}
// one DDV stage of a recorded sequence: every refusal comes before the launch
static int cos_op(const p2v_op& o, void* stream) {
  if (!o.in || !o.out || !o.lin.w_codes) return fail(P2V_E_ARG, "P2V_OP_COS: null buffer, partials or stage record");
  if ((uintptr_t)o.out % 8 || (uintptr_t)o.lin.w_codes % 8) return fail(P2V_E_ARG, "P2V_OP_COS: partials and stage record must be 8-byte aligned");
  const p2v_cos_layer l = cos_op_layer(o);
  const int rc = cos_check(&l, 1, o.i0, "P2V_OP_COS");
  if (rc != P2V_OK) return rc;
  const CosDesc d = p2v_cos_desc(l, o.i0, 0);
  return launch_rc(p2v_launch_cos_stage(reinterpret_cast<const CosDesc*>(o.lin.w_codes), (long long)o.i0 * d.nsplit,
                                        reinterpret_cast<unsigned long long*>(o.out), (hipStream_t)stream), "cos_stage");
}
static int cos_combine_op(const p2v_op& o, void* stream) {
  if (!o.in || !o.out || !o.lin.w_codes) return fail(P2V_E_ARG, "P2V_OP_COS_COMBINE: null stage table, sums or partials");
  if (o.i1 < 1) return fail(P2V_E_ARG, "P2V_OP_COS_COMBINE: a combine without stages (%d)", o.i1);
  if (o.i0 < 1) return fail(P2V_E_SHAPE, "P2V_OP_COS_COMBINE: n = %d samples", o.i0);
  if ((uintptr_t)o.in % 8 || (uintptr_t)o.out % 8 || (uintptr_t)o.lin.w_codes % 8) return fail(P2V_E_ARG, "P2V_OP_COS_COMBINE: pointers must be 8-byte aligned");
  return launch_rc(p2v_launch_cos_combine(reinterpret_cast<const CosDesc*>(o.in), o.i1, o.i0, reinterpret_cast<const unsigned long long*>(o.lin.w_codes),
                                          reinterpret_cast<double*>(o.out), (hipStream_t)stream), "cos_combine");
}
// one stage of the stage statistics in a recorded sequence (addressing in the members P2V_OP_COS uses): every refusal before the launch
static int stats_check(const p2v_stat_layer& a, const void* rec, bool aligned, const char* what, int l);
static int stats_op(const p2v_op& o, void* stream) {
  const long long sample = (long long)(((unsigned long long)(unsigned)o.i3 << 32) | (unsigned)o.i2);
  const p2v_stat_layer l{o.in, sample, o.lda, o.i0, o.M, o.N, o.i1};
  const int rc = stats_check(l, o.out, false, "P2V_OP_STATS", 0);
  return rc != P2V_OK ? rc : launch_rc(p2v_launch_stats(p2v_stats_desc(l, o.out), (hipStream_t)stream), "stats_stage");
}

static int run_one_op(const p2v_op& o, void* stream) {
  switch (o.kind) {
    case P2V_OP_PATCHIFY:
      return p2v_quantize_patchify((const float*)o.in, o.i0, o.i1, o.i2, o.i3, o.i4, o.f0, (int8_t*)o.out, o.i5, stream);
    case P2V_OP_GEMM:
      // REQUANT / GELU: ep.tap_out (fp32 layer output) goes through with the epilogue; RESID: the same member names the int8 mid codes
      return p2v_gemm_i8(o.epi, (const int8_t*)o.in, o.lda, o.M, o.K, o.N, &o.lin, &o.ep, o.out, o.ldo,
                         o.epi == P2V_EPI_RESID ? reinterpret_cast<int8_t*>(o.ep.tap_out) : nullptr, stream);
    case P2V_OP_LAYERNORM:
      return p2v_int_layernorm((const int8_t*)o.in, o.lda, o.M, o.N, &o.ln, (int8_t*)o.out, o.ldo, stream);
    case P2V_OP_WINATTN:
      // (additive) the planes of p2v_window_attention_taps in members this kind did not read before: all NULL = the untapped launch
      // (additive) i4: the softmax width, 0 = 4 (an earlier record)
      return p2v_window_attention_taps_bits((const int8_t*)o.in, o.i0, o.i1, o.i2, o.i3, &o.wa, o.i4 ? o.i4 : 4, (int8_t*)o.out,
                                            const_cast<int8_t*>(o.lin.w_codes), const_cast<int8_t*>(o.lin.w_frag),
                                            reinterpret_cast<int8_t*>(o.ep.tap_out), o.ldo, stream);
    case P2V_OP_MERGE:
      return p2v_patch_merge_gather((const int8_t*)o.in, o.i0, o.i1, o.i2, o.i3, (int8_t*)o.out, stream);
    case P2V_OP_AVGPOOL:
      return p2v_avgpool_quant((const int8_t*)o.in, o.i0, o.i1, o.i2, o.f0, o.f1, (int8_t*)o.out, stream);
    case P2V_OP_LN_GEMM:
      return p2v_ln_gemm_i8(o.epi, (const int8_t*)o.in, o.lda, o.M, o.K, &o.ln, o.N, &o.lin, &o.ep, (int8_t*)o.out, o.ldo, nullptr, stream);
    case P2V_OP_COS:
      return cos_op(o, stream);
    case P2V_OP_COS_COMBINE:
      return cos_combine_op(o, stream);
    case P2V_OP_GEMM_F32:
      return gemm_f32_op(o, stream);
    case P2V_OP_WINATTN_SOFTMAX:
      // P2V_OP_WINATTN's members; lin.w_codes (a tap plane there) names the softmax table
      return p2v_window_softmax_attention((const int8_t*)o.in, o.i0, o.i1, o.i2, o.i3, &o.wa, reinterpret_cast<const uint32_t*>(o.lin.w_codes),
                                          (int8_t*)o.out, stream);
    case P2V_OP_STATS:
      return stats_op(o, stream);
    case P2V_OP_FLOAT_LAYERNORM: {
      // P2V_OP_LAYERNORM's shape members; the constants in members no LayerNorm record read before (op table of include/p2vit.h)
      const p2v_float_ln f{o.f0, o.f1, reinterpret_cast<const float*>(o.lin.w_codes), o.lin.colscale, o.lin.bias};
      return p2v_float_layernorm((const int8_t*)o.in, o.lda, o.M, o.N, &f, (int8_t*)o.out, o.ldo, o.ep.tap_out, stream);
    }
    default:
      return fail(P2V_E_ARG, "p2v_run_ops: unknown op kind %d", o.kind);
  }
}

int p2v_run_ops(const p2v_op* ops, int n_ops, void* stream) {
  if (!ops || n_ops < 0) return fail(P2V_E_ARG, "p2v_run_ops: null argument");
  for (int i = 0; i < n_ops; ++i) {
    const int rc = run_one_op(ops[i], stream);
    if (rc != P2V_OK) return rc;
  }
  return P2V_OK;
}

int p2v_run_ops_profile(const p2v_op* ops, int n_ops, void* stream, float* ms) {
  if (!ops || !ms || n_ops < 0) return fail(P2V_E_ARG, "p2v_run_ops_profile: null argument");
  if (const int cap = refuse_capture("p2v_run_ops_profile", "times every record with events and synchronises the stream", stream)) return cap;
  hipStream_t st = (hipStream_t)stream;
  std::vector<hipEvent_t> ev(n_ops + 1);
  for (auto& e : ev) hipEventCreate(&e);
  int rc = P2V_OK;
  hipEventRecord(ev[0], st);
  int done = 0;
  for (; done < n_ops; ++done) {
    rc = run_one_op(ops[done], stream);
    if (rc != P2V_OK) break;
    hipEventRecord(ev[done + 1], st);
  }
  hipStreamSynchronize(st);
  for (int i = 0; i < done; ++i) hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
  for (auto& e : ev) hipEventDestroy(e);
  return rc;
}

int p2v_fake_quant_f32(const float* x, long long n, const float* scale, int n_scale, long long inner, int lo, int hi, float* out,
                       int8_t* codes, void* stream) {
  if (!x || !scale || (!out && !codes)) return fail(P2V_E_ARG, "p2v_fake_quant_f32: null argument");
  if (n_scale < 1 || inner < 1) return fail(P2V_E_ARG, "n_scale and inner must be >= 1");
  if (n == 0) return P2V_OK;
  return launch_rc(p2v_launch_fake_quant(x, n, scale, n_scale, inner, lo, hi, out, codes, (hipStream_t)stream), "fake_quant");
}

int p2v_gelu_quant_f32(const float* y, long long n, float inv_s, int8_t* codes, unsigned long long* flags, int force_slow,
                       void* stream) {
  if (!y || !codes) return fail(P2V_E_ARG, "p2v_gelu_quant_f32: null argument");
  if (n == 0) return P2V_OK;
  return launch_rc(p2v_launch_gelu_quant(y, n, inv_s, codes, flags, force_slow, (hipStream_t)stream), "gelu_quant");
}

int p2v_stream_probe(void* stream, int kernels, int usec, int workgroups, int lds_bytes) {
  if (kernels < 1 || kernels > 64 || usec < 1 || usec > 1000 || workgroups < 1 || workgroups > 4096 || lds_bytes < 0 || lds_bytes > 65536)
    return fail(P2V_E_ARG, "p2v_stream_probe: 1..64 kernels of 1..1000 us, 1..4096 workgroups, 0..64 KB of LDS");
  return launch_rc(p2v_launch_stream_probe(kernels, usec, workgroups, lds_bytes, (hipStream_t)stream), "stream_probe");
}

#ifdef P2V_DIAG
/* diagnostic build only (make diag): device buffer receiving 6 x uint64 per workgroup of the next tiled GEMM launches */
extern unsigned long long* g_gemm_stamps;
void p2v_debug_set_gemm_stamps(void* dev) { g_gemm_stamps = (unsigned long long*)dev; }
#endif

int p2v_gelu_table_plan(float inv_s, p2v_gelu_tab* t) {
  if (!t) return fail(P2V_E_ARG, "p2v_gelu_table_plan: null argument");
  if (!is_pot(inv_s) || inv_s < 1.0f || inv_s > 4096.0f) return fail(P2V_E_UNSUPPORTED, "gelu table: 1/scale %g is not a power of two in [1, 4096]", inv_s);
  const double s = 1.0 / (double)inv_s, k = 2.0 * (double)inv_s;          // cells of width s/2
  // below y_lo every code is 0: |gelu(y)| = 0.5 |y| erfc(|y|/sqrt 2) falls monotonically left of the minimum at -0.7518
  double y_lo = -0.75;
  while (y_lo > -40.0 && 0.5 * -y_lo * erfc(-y_lo * 0.70710678118654752440) >= 0.25 * s) y_lo -= 0.5 * s;
  const long long i0 = (long long)floor((y_lo - s) * k);
  double y_hi = 127.5 * s;                                                  // gelu(y) < y: the code saturates at 127 a little later
  while (y_hi < 1.0e4 && 0.5 * y_hi * erfc(-y_hi * 0.70710678118654752440) < 127.75 * s) y_hi += 0.5 * s;
  const long long i1 = (long long)ceil(y_hi * k) + 2;                       // from here on every code is 127
  const long long cells = i1 - i0;
  if (cells > 4096) return fail(P2V_E_UNSUPPORTED, "gelu table: %lld cells for 1/scale %g (limit 4096)", cells, inv_s);
  t->k = (float)k;
  t->off = (float)(-i0);
  t->cells = (int32_t)cells;
  return P2V_OK;
}

size_t p2v_gelu_table_scratch_bytes(int cells) { return cells > 0 ? ((size_t)4 * cells + 4) * 4 : 0; }

int p2v_gelu_table_build(float inv_s, const p2v_gelu_tab* t, void* scratch, size_t scratch_bytes, void* stream) {
  if (!t || !t->table || !scratch) return fail(P2V_E_ARG, "p2v_gelu_table_build: null argument");
  p2v_gelu_tab want;
  const int rc = p2v_gelu_table_plan(inv_s, &want);
  if (rc != P2V_OK) return rc;
  if (want.k != t->k || want.off != t->off || want.cells != t->cells) return fail(P2V_E_ARG, "p2v_gelu_table_build: descriptor does not come from p2v_gelu_table_plan");
  if (scratch_bytes < p2v_gelu_table_scratch_bytes(t->cells)) return fail(P2V_E_WORKSPACE, "gelu table scratch %zu < %zu bytes", scratch_bytes, p2v_gelu_table_scratch_bytes(t->cells));
  if (const int cap = refuse_capture("p2v_gelu_table_build", "reads the build status back to the host", stream)) return cap;
  hipStream_t st = (hipStream_t)stream;
  const int lrc = launch_rc(p2v_launch_gelu_table_build(inv_s, *t, (unsigned*)scratch, st), "gelu_table_build");
  if (lrc != P2V_OK) return lrc;
  unsigned status = 0;
  hipError_t e = hipMemcpyAsync(&status, (const unsigned*)scratch + 4 * t->cells, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(P2V_E_LAUNCH, "gelu_table_build: %s", hipGetErrorString(e));
  if (status) return fail(P2V_E_UNSUPPORTED, "gelu table for 1/scale %g: %s", inv_s, (status & 1) ? "a cell holds two thresholds" : "a cell is never hit");
  return P2V_OK;
}

int p2v_gelu_table_check(float inv_s, const p2v_gelu_tab* t, unsigned long long* mismatches, void* stream) {
  if (!t || !t->table || !mismatches) return fail(P2V_E_ARG, "p2v_gelu_table_check: null argument");
  if (t->cells <= 0) return fail(P2V_E_ARG, "p2v_gelu_table_check: empty table");
  return launch_rc(p2v_launch_gelu_table_check(inv_s, *t, mismatches, (hipStream_t)stream), "gelu_table_check");
}

int p2v_gelu_err_sweep(unsigned first_bits, unsigned count, float* max_err, void* stream) {
  if (!max_err) return fail(P2V_E_ARG, "p2v_gelu_err_sweep: null argument");
  return launch_rc(p2v_launch_gelu_sweep(first_bits, count, max_err, (hipStream_t)stream), "gelu_sweep");
}

}  // extern "C"

// ---- CKA model diff (p2vit_cka.hip) ------------------------------------------------------------------------------------------------
static int cka_check(const p2v_cka_layer* layers, int n_layers, int n, const char* what) {
  if (!layers || n_layers <= 0) return fail(P2V_E_ARG, "%s: no layers", what);
  if (n < P2V_CKA_MIN_N || n > P2V_CKA_MAX_N) return fail(P2V_E_SHAPE, "%s: n = %d images, the kernels take %d ... %d", what, n, P2V_CKA_MIN_N, P2V_CKA_MAX_N);
  for (int l = 0; l < n_layers; ++l) {
    const p2v_cka_layer& a = layers[l];
    if (!a.x) return fail(P2V_E_ARG, "%s: layer %d has a null x", what, l);
    if (a.features < 1 || a.ldx < a.features) return fail(P2V_E_ARG, "%s: layer %d: F = %lld, ldx = %lld", what, l, a.features, a.ldx);
    if (a.y && a.y != a.x && a.ldy < a.features) return fail(P2V_E_ARG, "%s: layer %d: ldy = %lld < F", what, l, a.ldy);
  }
  return P2V_OK;
}

size_t p2v_cka_workspace_bytes(const p2v_cka_layer* layers, int n_layers, int n) {
  if (cka_check(layers, n_layers, n, "p2v_cka_workspace_bytes") != P2V_OK) return 0;
  return p2v_cka_layout(layers, n_layers, n, nullptr).total;
}

int p2v_cka_grams(const p2v_cka_layer* layers, int n_layers, int n, float* grams, void* ws, size_t ws_bytes, void* stream) {
  int rc = cka_check(layers, n_layers, n, "p2v_cka_grams");
  if (rc != P2V_OK) return rc;
  if (!grams || !ws) return fail(P2V_E_ARG, "p2v_cka_grams: null grams / workspace");
  std::vector<CkaDesc> descs;
  descs.reserve(n_layers);
  const CkaLayout w = p2v_cka_layout(layers, n_layers, n, &descs);
  if (ws_bytes < w.total) return fail(P2V_E_WORKSPACE, "p2v_cka_grams: workspace %zu < %zu bytes", ws_bytes, w.total);
  if ((uintptr_t)ws % 256) return fail(P2V_E_ARG, "p2v_cka_grams: the workspace must be 256-byte aligned");
  if (const int cap = refuse_capture("p2v_cka_grams", "uploads its layer descriptors from a host array that does not outlive it", stream)) return cap;
  return launch_rc(p2v_launch_cka_grams(descs, w, n, grams, ws, (hipStream_t)stream), "cka_grams");
}

int p2v_hsic_accumulate(const float* g1, int l1, const float* g2, int l2, int n, void* acc, void* self1, void* self2, int dtype,
                        void* stream) {
  if (!g1 || !g2 || !acc || l1 <= 0 || l2 <= 0) return fail(P2V_E_ARG, "p2v_hsic_accumulate: null gram / accumulator or no layers");
  if (n < P2V_CKA_MIN_N || n > P2V_CKA_MAX_N) return fail(P2V_E_SHAPE, "p2v_hsic_accumulate: n = %d images, the kernels take %d ... %d", n, P2V_CKA_MIN_N, P2V_CKA_MAX_N);
  if (dtype != 0 && dtype != 1) return fail(P2V_E_ARG, "p2v_hsic_accumulate: dtype %d (0 = fp32, 1 = fp64)", dtype);
  return launch_rc(p2v_launch_hsic(g1, l1, g2, l2, n, acc, self1, self2, dtype, (hipStream_t)stream), "hsic_accumulate");
}

// ---- DDV model diff (p2vit_ddv.hip) ------------------------------------------------------------------------------------------------
static int cos_check(const p2v_cos_layer* layers, int n_layers, int n, const char* what) {
  if (!layers || n_layers <= 0) return fail(P2V_E_ARG, "%s: no layers", what);
  if (n < 1) return fail(P2V_E_SHAPE, "%s: n = %d samples", what, n);
  for (int l = 0; l < n_layers; ++l) {
    const p2v_cos_layer& a = layers[l];
    if (!a.a || !a.b) return fail(P2V_E_ARG, "%s: layer %d has a null operand", what, l);
    if (a.dtype != P2V_COS_I8 && a.dtype != P2V_COS_F32 && a.dtype != P2V_COS_LOG2K)
      return fail(P2V_E_ARG, "%s: layer %d: dtype %d (0 = int8, 1 = fp32, 3 = log2 exponents)", what, l, a.dtype);
    if (a.scale && a.dtype == P2V_COS_LOG2K) return fail(P2V_E_ARG, "%s: layer %d: the log2-exponent form takes no scales", what, l);
    if (a.rows < 1 || a.cols < 1) return fail(P2V_E_SHAPE, "%s: layer %d: %d rows x %d cols", what, l, a.rows, a.cols);
    if (a.row_stride < a.cols) return fail(P2V_E_ARG, "%s: layer %d: row_stride %lld < cols %d", what, l, a.row_stride, a.cols);
    if (a.sample_stride < 0) return fail(P2V_E_ARG, "%s: layer %d: negative sample_stride %lld", what, l, a.sample_stride);
    if (a.scale && a.dtype != P2V_COS_I8) return fail(P2V_E_UNSUPPORTED, "%s: layer %d: per-channel scales go with int8 codes", what, l);
    const long long esz = a.dtype == P2V_COS_F32 ? 4 : 1;
    if ((uintptr_t)a.a % 16 || (uintptr_t)a.b % 16 || a.sample_stride * esz % 16 || a.row_stride * esz % 16)
      return fail(P2V_E_ARG, "%s: layer %d: pointers and strides must be multiples of 16 bytes", what, l);
    if (a.dtype == P2V_COS_I8 && (long long)a.rows * a.cols >= (1LL << 39))
      return fail(P2V_E_UNSUPPORTED, "%s: layer %d: %d x %d codes per sample leave the exact fp64 range", what, l, a.rows, a.cols);
    if (a.dtype == P2V_COS_LOG2K && (long long)a.rows * a.cols >= (1LL << 33))       // 2^30 per element: the int64 sums cannot overflow below this
      return fail(P2V_E_UNSUPPORTED, "%s: layer %d: %d x %d exponents per sample", what, l, a.rows, a.cols);
  }
  return P2V_OK;
}

size_t p2v_pair_cosine_workspace_bytes(const p2v_cos_layer* layers, int n_layers, int n) {
  if (cos_check(layers, n_layers, n, "p2v_pair_cosine_workspace_bytes") != P2V_OK) return 0;
  return p2v_cos_layout(layers, n_layers, n, nullptr).total;
}

int p2v_pair_cosine(const p2v_cos_layer* layers, int n_layers, int n, double* sums, void* ws, size_t ws_bytes, void* stream) {
  int rc = cos_check(layers, n_layers, n, "p2v_pair_cosine");
  if (rc != P2V_OK) return rc;
  if (!sums || !ws) return fail(P2V_E_ARG, "p2v_pair_cosine: null sums / workspace");
  std::vector<CosDesc> descs;
  descs.reserve(n_layers);
  const CosLayout w = p2v_cos_layout(layers, n_layers, n, &descs);
  if (ws_bytes < w.total) return fail(P2V_E_WORKSPACE, "p2v_pair_cosine: workspace %zu < %zu bytes", ws_bytes, w.total);
  if ((uintptr_t)ws % 256) return fail(P2V_E_ARG, "p2v_pair_cosine: the workspace must be 256-byte aligned");
  if (const int cap = refuse_capture("p2v_pair_cosine", "uploads its layer descriptors from a host array that does not outlive it", stream)) return cap;
  return launch_rc(p2v_launch_pair_cosine(descs, w, n, sums, ws, (hipStream_t)stream), "pair_cosine");
}

// stage records of a recorded DDV sequence (P2V_OP_COS / P2V_OP_COS_COMBINE): built once on the host, uploaded by the caller
size_t p2v_cos_stage_desc_bytes(void) { return sizeof(CosDesc); }

long long p2v_cos_stage_descs(const p2v_cos_layer* layers, int n_layers, int n, void* host_descs) {
  const int rc = cos_check(layers, n_layers, n, "p2v_cos_stage_descs");
  if (rc != P2V_OK) return rc;
  if (!host_descs) return fail(P2V_E_ARG, "p2v_cos_stage_descs: null output");
  std::vector<CosDesc> descs;
  descs.reserve(n_layers);
  const CosLayout w = p2v_cos_layout(layers, n_layers, n, &descs);
  if (w.items >= (1LL << 31)) return fail(P2V_E_UNSUPPORTED, "p2v_cos_stage_descs: %lld partials", w.items);
  memcpy(host_descs, descs.data(), descs.size() * sizeof(CosDesc));
  return w.items;
}

// ---- stage statistics (p2vit_stats.hip) ------------------------------------------------------------------------------------------------
// aligned: the public rule (base and strides multiples of 16 bytes); the forward's own stages (logits of a class count that is no multiple
// of 4) pass false and read with scalar loads
static int stats_check(const p2v_stat_layer& a, const void* rec, bool aligned, const char* what, int l) {
  if (!a.base || !rec) return fail(P2V_E_ARG, "%s: layer %d has a null plane or record", what, l);
  if (a.dtype != P2V_STAT_I8 && a.dtype != P2V_STAT_F32 && a.dtype != P2V_STAT_U8)
    return fail(P2V_E_ARG, "%s: layer %d: dtype %d (0 = int8, 1 = fp32, 2 = uint8)", what, l, a.dtype);
  if (a.cols < 1) return fail(P2V_E_SHAPE, "%s: layer %d: %d cols", what, l, a.cols);
  if (a.rows < 0 || a.samples < 0) return fail(P2V_E_ARG, "%s: layer %d: %d samples x %d rows", what, l, a.samples, a.rows);
  if (a.row_stride < a.cols) return fail(P2V_E_ARG, "%s: layer %d: row_stride %lld < cols %d", what, l, a.row_stride, a.cols);
  if (a.sample_stride < 0) return fail(P2V_E_ARG, "%s: layer %d: negative sample_stride %lld", what, l, a.sample_stride);
  const long long esz = a.dtype == P2V_STAT_F32 ? 4 : 1;
  if (aligned && ((uintptr_t)a.base % 16 || a.sample_stride * esz % 16 || a.row_stride * esz % 16))
    return fail(P2V_E_ARG, "%s: layer %d: pointers and strides must be multiples of 16 bytes", what, l);
  if ((uintptr_t)a.base % esz) return fail(P2V_E_ARG, "%s: layer %d: the plane is not aligned to its element", what, l);
  if ((uintptr_t)rec % 16) return fail(P2V_E_ARG, "%s: layer %d: the record must be 16-byte aligned", what, l);
  if ((long long)a.samples * a.rows >= (1LL << 31))
    return fail(P2V_E_UNSUPPORTED, "%s: layer %d: %d samples x %d rows", what, l, a.samples, a.rows);
  return P2V_OK;
}

size_t p2v_stats_bytes(int cols) { return cols < 1 ? 0 : ((size_t)2080 + (size_t)24 * cols + 15) / 16 * 16; }

int p2v_stats_init(void* out, size_t bytes, int dtype, int cols, void* stream) {
  if (!out) return fail(P2V_E_ARG, "p2v_stats_init: null record");
  if (dtype != P2V_STAT_I8 && dtype != P2V_STAT_F32 && dtype != P2V_STAT_U8)
    return fail(P2V_E_ARG, "p2v_stats_init: dtype %d (0 = int8, 1 = fp32, 2 = uint8)", dtype);
  if (cols < 1 || cols > (1 << 26)) return fail(P2V_E_SHAPE, "p2v_stats_init: %d cols", cols);
  if ((uintptr_t)out % 16) return fail(P2V_E_ARG, "p2v_stats_init: the record must be 16-byte aligned");
  if (bytes < p2v_stats_bytes(cols)) return fail(P2V_E_WORKSPACE, "p2v_stats_init: record %zu < %zu bytes", bytes, p2v_stats_bytes(cols));
  return launch_rc(p2v_launch_stats_init(out, p2v_stats_bytes(cols), dtype, cols, (hipStream_t)stream), "stats_init");
}

int p2v_code_stats(const p2v_stat_layer* layers, int n_layers, void* const* records, void* ws, size_t ws_bytes, void* stream) {
  (void)ws; (void)ws_bytes;
  if (!layers || !records || n_layers <= 0) return fail(P2V_E_ARG, "p2v_code_stats: no layers");
  for (int l = 0; l < n_layers; ++l) {
    const int rc = stats_check(layers[l], records[l], true, "p2v_code_stats", l);
    if (rc != P2V_OK) return rc;
  }
  for (int l = 0; l < n_layers; ++l) {
    const int rc = launch_rc(p2v_launch_stats(p2v_stats_desc(layers[l], records[l]), (hipStream_t)stream), "code_stats");
    if (rc != P2V_OK) return rc;
  }
  return P2V_OK;
}

// ---- scoring of the logits (p2vit_score.hip) -------------------------------------------------------------------------------------------
int p2v_score_logits(const float* logits, long long ld, int rows, int classes, const long long* labels, int32_t* ranks, double* loss,
                     void* stream) {
  if (!logits || !labels || !ranks || !loss) return fail(P2V_E_ARG, "p2v_score_logits: null argument");
  if (rows < 0 || classes < 1 || ld < classes) return fail(P2V_E_ARG, "p2v_score_logits: rows %d, classes %d, ld %lld", rows, classes, ld);
  if (rows == 0) return P2V_OK;
  return launch_rc(p2v_launch_score_rows(logits, ld, rows, classes, labels, ranks, loss, (hipStream_t)stream), "score_logits");
}

size_t p2v_score_totals_bytes(int n_k) { return n_k < 1 || n_k > P2V_SCORE_MAX_K ? 0 : (size_t)(3 + 3 * n_k) * 8; }

int p2v_score_accumulate(const int32_t* ranks, const double* loss, int rows, const int* ks, int n_k, void* totals_slot, void* stream) {
  if (!ranks || !loss || !ks || !totals_slot) return fail(P2V_E_ARG, "p2v_score_accumulate: null argument");
  if (rows < 0) return fail(P2V_E_ARG, "p2v_score_accumulate: rows %d", rows);
  if (n_k < 1 || n_k > P2V_SCORE_MAX_K) return fail(P2V_E_ARG, "p2v_score_accumulate: %d values of k (1 ... %d)", n_k, P2V_SCORE_MAX_K);
  for (int q = 0; q < n_k; ++q)
    if (ks[q] < 1) return fail(P2V_E_ARG, "p2v_score_accumulate: k = %d", ks[q]);
  if ((uintptr_t)totals_slot % 8) return fail(P2V_E_ARG, "p2v_score_accumulate: the totals slot must be 8-byte aligned");
  if (rows == 0) return P2V_OK;
  return launch_rc(p2v_launch_score_accumulate(ranks, loss, rows, ks, n_k, totals_slot, (hipStream_t)stream), "score_accumulate");
}

// ---- search-based profiling inputs (p2vit_profile.hip) ---------------------------------------------------------------------------------
static bool prof_sizes_ok(int n, int classes) { return n >= 1 && n <= P2V_PROFILE_MAX_N && classes >= 1 && classes <= P2V_PROFILE_MAX_CLASSES; }

size_t p2v_profile_state_bytes(int n, int classes) { return prof_sizes_ok(n, classes) ? (size_t)p2v_profile_layout(n, classes).bytes : 0; }

static int prof_state_check(const char* who, const void* state, size_t state_bytes, int n, int classes) {
  if (!state) return fail(P2V_E_ARG, "%s: null state block", who);
  if ((uintptr_t)state % 16) return fail(P2V_E_ARG, "%s: the state block must be 16-byte aligned", who);
  if (!prof_sizes_ok(n, classes))
    return fail(P2V_E_SHAPE, "%s: n %d (1 ... %d), classes %d (1 ... %d)", who, n, P2V_PROFILE_MAX_N, classes, P2V_PROFILE_MAX_CLASSES);
  if (state_bytes < p2v_profile_state_bytes(n, classes))
    return fail(P2V_E_WORKSPACE, "%s: state block %zu < %zu bytes", who, state_bytes, p2v_profile_state_bytes(n, classes));
  return P2V_OK;
}

static int prof_image_check(const char* who, int n, long long image_elems, int idx, long long pos) {
  if (n < 1 || n > P2V_PROFILE_MAX_N || image_elems < 1 || image_elems > (1LL << 30))
    return fail(P2V_E_SHAPE, "%s: n %d (1 ... %d), image_elems %lld (1 ... 2^30)", who, n, P2V_PROFILE_MAX_N, image_elems);
  if (idx < 0 || idx >= n) return fail(P2V_E_ARG, "%s: idx %d outside [0, %d)", who, idx, n);
  if (pos < 0 || pos >= image_elems) return fail(P2V_E_ARG, "%s: pos %lld outside [0, %lld)", who, pos, image_elems);
  return P2V_OK;
}

int p2v_profile_init(void* state, size_t state_bytes, int n, int classes, const float* logits1, const float* logits2, void* stream) {
  if (!logits1 || !logits2) return fail(P2V_E_ARG, "p2v_profile_init: null logits");
  if ((uintptr_t)logits1 % 4 || (uintptr_t)logits2 % 4) return fail(P2V_E_ARG, "p2v_profile_init: logits must be 4-byte aligned");
  const int rc = prof_state_check("p2v_profile_init", state, state_bytes, n, classes);
  if (rc != P2V_OK) return rc;
  return launch_rc(p2v_launch_profile_init(state, n, classes, logits1, logits2, (hipStream_t)stream), "profile_init");
}

int p2v_profile_candidates(const float* inputs, int n, long long image_elems, int idx, long long pos, float epsilon, float* staging,
                           void* stream) {
  if (!inputs || !staging) return fail(P2V_E_ARG, "p2v_profile_candidates: null argument");
  if ((uintptr_t)inputs % 16 || (uintptr_t)staging % 16) return fail(P2V_E_ARG, "p2v_profile_candidates: inputs and staging must be 16-byte aligned");
  const int rc = prof_image_check("p2v_profile_candidates", n, image_elems, idx, pos);
  if (rc != P2V_OK) return rc;
  return launch_rc(p2v_launch_profile_candidates(inputs, image_elems, idx, pos, epsilon, staging, (hipStream_t)stream), "profile_candidates");
}

int p2v_profile_step(void* state, size_t state_bytes, int n, int classes, const float* cand1, const float* cand2, const float* staging,
                     float* inputs, long long image_elems, int idx, long long pos, double* trace_row, void* stream) {
  if (!cand1 || !cand2 || !staging || !inputs || !trace_row) return fail(P2V_E_ARG, "p2v_profile_step: null argument");
  if ((uintptr_t)cand1 % 4 || (uintptr_t)cand2 % 4) return fail(P2V_E_ARG, "p2v_profile_step: candidate logits must be 4-byte aligned");
  if ((uintptr_t)inputs % 16 || (uintptr_t)staging % 16) return fail(P2V_E_ARG, "p2v_profile_step: inputs and staging must be 16-byte aligned");
  if ((uintptr_t)trace_row % 8) return fail(P2V_E_ARG, "p2v_profile_step: the trace row must be 8-byte aligned");
  int rc = prof_state_check("p2v_profile_step", state, state_bytes, n, classes);
  if (rc != P2V_OK) return rc;
  rc = prof_image_check("p2v_profile_step", n, image_elems, idx, pos);
  if (rc != P2V_OK) return rc;
  return launch_rc(p2v_launch_profile_step(state, n, classes, cand1, cand2, staging, inputs, image_elems, idx, pos, trace_row,
                                           (hipStream_t)stream), "profile_step");
}

int p2v_profile_diversity(const float* logits, long long ld, int n, int classes, double* out, void* ws, size_t ws_bytes, void* stream) {
  if (!logits || !out || !ws) return fail(P2V_E_ARG, "p2v_profile_diversity: null argument");
  if ((uintptr_t)logits % 4 || (uintptr_t)out % 8 || (uintptr_t)ws % 8)
    return fail(P2V_E_ARG, "p2v_profile_diversity: logits must be 4-byte, out and ws 8-byte aligned");
  if (!prof_sizes_ok(n, classes) || ld < classes)
    return fail(P2V_E_SHAPE, "p2v_profile_diversity: n %d (1 ... %d), classes %d (1 ... %d), ld %lld", n, P2V_PROFILE_MAX_N, classes,
                P2V_PROFILE_MAX_CLASSES, ld);
  if (ws_bytes < (size_t)n * n * 8) return fail(P2V_E_WORKSPACE, "p2v_profile_diversity: workspace %zu < %zu bytes", ws_bytes, (size_t)n * n * 8);
  return launch_rc(p2v_launch_profile_diversity(logits, ld, n, classes, reinterpret_cast<double*>(ws), out, (hipStream_t)stream),
                   "profile_diversity");
}

int p2v_ddv_stage_count_ex(const p2v_plan* plan, int with_linear, int stage_set) {
  if (!plan) return fail(P2V_E_ARG, "p2v_ddv_stage_count: null plan");
  if (stage_set != P2V_DDV_STAGES_ENGINE && stage_set != P2V_DDV_STAGES_FULL)
    return fail(P2V_E_ARG, "p2v_ddv_stage_count_ex: unknown stage_set %d (P2V_DDV_STAGES_ENGINE = 0, P2V_DDV_STAGES_FULL = 1)", stage_set);
  return 5 * plan->d.depth + 3 + (with_linear ? 4 * plan->d.depth + 1 : 0) + (stage_set == P2V_DDV_STAGES_FULL ? 4 * plan->d.depth + 4 : 0);
}
int p2v_ddv_stage_count(const p2v_plan* plan, int with_linear) { return p2v_ddv_stage_count_ex(plan, with_linear, P2V_DDV_STAGES_ENGINE); }
int p2v_ddv_stage_count_ex2(const p2v_plan* plan, int with_linear, int stage_set) {
  if (!plan) return fail(P2V_E_ARG, "p2v_ddv_stage_count: null plan");
  if (stage_set < 0 || stage_set > (P2V_DDV_STAGES_FULL | P2V_DDV_STAGES_ATTN))
    return fail(P2V_E_ARG, "p2v_ddv_stage_count_ex2: unknown stage_set %d (ENGINE = 0 or FULL = 1, optionally | P2V_DDV_STAGES_ATTN = 2)", stage_set);
  const int base = p2v_ddv_stage_count_ex(plan, with_linear, stage_set & ~P2V_DDV_STAGES_ATTN);
  return base < 0 ? base : base + ((stage_set & P2V_DDV_STAGES_ATTN) ? 2 * plan->d.depth : 0);
}

// workgroups of the largest stage: p2v_cos_desc gives a sample at most 2048 / n (>= 1) splits while its rows stay below 2^16 per split -
// true of every stage here (at most 4096 tokens); ddv_reduce checks each stage against this count before it launches
static long long ddv_partial_slots(int n) { return n > 2048 ? n : 2048; }
static size_t ddv_partial_bytes(int n) { return (size_t)ddv_partial_slots(n) * 3 * sizeof(unsigned long long); }

// (the FULL stages live in buffers of the forward's workspace that are free where they are taken: the size does not depend on the stage set)
size_t p2v_ddv_workspace_bytes_ex(const p2v_plan* plan, int n, int stage_set) {
  if (!plan || n <= 0 || n > (1 << 29) || (stage_set != P2V_DDV_STAGES_ENGINE && stage_set != P2V_DDV_STAGES_FULL)) return 0;
  return ws_layout(plan, 2 * n).total + ddv_partial_bytes(n);        // (the forward's part is a multiple of 256 bytes)
}
size_t p2v_ddv_workspace_bytes(const p2v_plan* plan, int n) { return p2v_ddv_workspace_bytes_ex(plan, n, P2V_DDV_STAGES_ENGINE); }

size_t p2v_ddv_tap_scratch_bytes(const p2v_plan* plan, int n) {
  if (!plan || n <= 0 || n > (1 << 29)) return 0;
  const size_t wide = (size_t)(3 * plan->d.embed_dim > plan->d.mlp_hidden ? 3 * plan->d.embed_dim : plan->d.mlp_hidden);
  const size_t tok = (size_t)2 * n * plan->tokens * wide, head = (size_t)2 * n * plan->d.num_classes;
  return (tok > head ? tok : head) * sizeof(float);
}

// bytes of the two attention planes (score codes, exponents) of the 2n images of ONE block, rows pitched to whole 16-byte groups
size_t p2v_ddv_attn_scratch_bytes(const p2v_plan* plan, int n) {
  if (!plan || n <= 0 || n > (1 << 29)) return 0;
  return (size_t)2 * 2 * n * plan->d.num_heads * plan->tokens * round_up(plan->tokens, 16);
}

static int forward_ddv_impl(p2v_plan* plan, const float* images, int n, const int8_t* bit_config, int n_cfg, float* logits, void* ws,
                            size_t ws_bytes, int with_linear, int stage_set, float* tap_scratch, size_t tap_scratch_bytes, int8_t* attn_scratch,
                            double* sums, void* stream) {
  if (!plan || !sums || !ws) return fail(P2V_E_ARG, "p2v_forward_ddv: null argument");
  if (stage_set != P2V_DDV_STAGES_ENGINE && stage_set != P2V_DDV_STAGES_FULL)
    return fail(P2V_E_ARG, "p2v_forward_ddv_ex: unknown stage_set %d (P2V_DDV_STAGES_ENGINE = 0, P2V_DDV_STAGES_FULL = 1)", stage_set);
  const bool full = stage_set == P2V_DDV_STAGES_FULL;
  if (n <= 0 || n > (1 << 29)) return fail(P2V_E_SHAPE, "p2v_forward_ddv: n = %d pairs", n);
  if ((uintptr_t)ws % 256) return fail(P2V_E_ARG, "p2v_forward_ddv: the workspace must be 256-byte aligned");
  if (full && !(plan->inv_s_input > 0.f))
    return fail(P2V_E_UNSUPPORTED, "p2v_forward_ddv_ex: the FULL stage set needs the input QAct (input_quant = False has no qact_input stage)");
  if (full && !plan->embed_cls_codes)
    return fail(P2V_E_STATE, "p2v_forward_ddv_ex: the FULL stage set needs the class row of qact_embed (p2v_plan_set_embed_tap_cls)");
  const size_t fwd = ws_layout(plan, 2 * n).total;
  if (ws_bytes < fwd + ddv_partial_bytes(n)) return fail(P2V_E_WORKSPACE, "p2v_forward_ddv: workspace %zu < %zu bytes", ws_bytes, fwd + ddv_partial_bytes(n));
  if (full && !tap_scratch)
    return fail(P2V_E_WORKSPACE, "p2v_forward_ddv_ex: the FULL stage set needs tap_scratch (%zu bytes) whatever with_linear says", p2v_ddv_tap_scratch_bytes(plan, n));
  if (with_linear || full) {
    if (!tap_scratch) return fail(P2V_E_ARG, "p2v_forward_ddv: with_linear needs tap_scratch");
    if ((uintptr_t)tap_scratch % 16) return fail(P2V_E_ARG, "p2v_forward_ddv: tap_scratch must be 16-byte aligned");
    if (tap_scratch_bytes < p2v_ddv_tap_scratch_bytes(plan, n))
      return fail(P2V_E_WORKSPACE, "p2v_forward_ddv: tap_scratch %zu < %zu bytes", tap_scratch_bytes, p2v_ddv_tap_scratch_bytes(plan, n));
  }
  DdvCtx ctx{n, reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(ws) + fwd), ddv_partial_slots(n), sums,
             with_linear ? tap_scratch : nullptr, 0};
  ctx.scratch = full ? tap_scratch : nullptr;
  ctx.attn = attn_scratch;
  std::vector<float*> taps;
  if (with_linear) {
    taps.assign(plan->n_layers, tap_scratch);      // every linear output goes through the one buffer; the patch embedding is no DDV stage
    taps[0] = nullptr;
  }
  FwdOpts o;
  o.images = images; o.ddv = &ctx; o.lin_tap = with_linear ? taps.data() : nullptr;
  return forward_impl(plan, 2 * n, bit_config, n_cfg, logits, ws, fwd, stream, o);
}

int p2v_forward_ddv_ex(p2v_plan* plan, const float* images, int n, const int8_t* bit_config, int n_cfg, float* logits, void* ws,
                       size_t ws_bytes, int with_linear, int stage_set, float* tap_scratch, size_t tap_scratch_bytes, double* sums, void* stream) {
  return forward_ddv_impl(plan, images, n, bit_config, n_cfg, logits, ws, ws_bytes, with_linear, stage_set, tap_scratch, tap_scratch_bytes, nullptr,
                          sums, stream);
}

// the stage sets with P2V_DDV_STAGES_ATTN or-ed on: the flag's own refusals first (before any launch), the rest is p2v_forward_ddv_ex's
int p2v_forward_ddv_ex2(p2v_plan* plan, const float* images, int n, const int8_t* bit_config, int n_cfg, float* logits, void* ws,
                        size_t ws_bytes, int with_linear, int stage_set, float* tap_scratch, size_t tap_scratch_bytes, int8_t* attn_scratch,
                        size_t attn_scratch_bytes, double* sums, void* stream) {
  if (stage_set < 0 || stage_set > (P2V_DDV_STAGES_FULL | P2V_DDV_STAGES_ATTN))
    return fail(P2V_E_ARG, "p2v_forward_ddv_ex2: unknown stage_set %d (ENGINE = 0 or FULL = 1, optionally | P2V_DDV_STAGES_ATTN = 2)", stage_set);
  if (!(stage_set & P2V_DDV_STAGES_ATTN))
    return forward_ddv_impl(plan, images, n, bit_config, n_cfg, logits, ws, ws_bytes, with_linear, stage_set, tap_scratch, tap_scratch_bytes, nullptr,
                            sums, stream);
  if (!plan) return fail(P2V_E_ARG, "p2v_forward_ddv_ex2: null argument");
  const size_t need = p2v_ddv_attn_scratch_bytes(plan, n);
  if (n <= 0 || !need) return fail(P2V_E_SHAPE, "p2v_forward_ddv: n = %d pairs", n);
  if (!attn_scratch) return fail(P2V_E_ARG, "p2v_forward_ddv_ex2: P2V_DDV_STAGES_ATTN needs attn_scratch (%zu bytes)", need);
  if ((uintptr_t)attn_scratch % 16) return fail(P2V_E_ARG, "p2v_forward_ddv_ex2: attn_scratch must be 16-byte aligned");
  if (attn_scratch_bytes < need) return fail(P2V_E_WORKSPACE, "p2v_forward_ddv_ex2: attn_scratch %zu < %zu bytes", attn_scratch_bytes, need);
  return forward_ddv_impl(plan, images, n, bit_config, n_cfg, logits, ws, ws_bytes, with_linear, stage_set & ~P2V_DDV_STAGES_ATTN, tap_scratch,
                          tap_scratch_bytes, attn_scratch, sums, stream);
}

int p2v_forward_ddv(p2v_plan* plan, const float* images, int n, const int8_t* bit_config, int n_cfg, float* logits, void* ws,
                    size_t ws_bytes, int with_linear, float* tap_scratch, size_t tap_scratch_bytes, double* sums, void* stream) {
  return p2v_forward_ddv_ex(plan, images, n, bit_config, n_cfg, logits, ws, ws_bytes, with_linear, P2V_DDV_STAGES_ENGINE, tap_scratch,
                            tap_scratch_bytes, sums, stream);
}

// ---- stage statistics inside the fused forward: p2v_forward_ddv_ex2's sequence, stage sets and refusals, with every stage site reducing all
// `batch` samples into its record (DdvCtx::stats) ------------------------------------------------------------------------------------------
static int stats_stage_set_check(const p2v_plan* plan, int stage_set, const char* who) {
  if (!plan) return fail(P2V_E_ARG, "%s: null argument", who);
  if (stage_set < 0 || stage_set > (P2V_DDV_STAGES_FULL | P2V_DDV_STAGES_ATTN))
    return fail(P2V_E_ARG, "%s: unknown stage_set %d (ENGINE = 0 or FULL = 1, optionally | P2V_DDV_STAGES_ATTN = 2)", who, stage_set);
  if ((stage_set & P2V_DDV_STAGES_FULL) && !(plan->inv_s_input > 0.f))
    return fail(P2V_E_UNSUPPORTED, "%s: the FULL stage set needs the input QAct (input_quant = False has no qact_input stage)", who);
  if ((stage_set & P2V_DDV_STAGES_FULL) && !plan->embed_cls_codes)
    return fail(P2V_E_STATE, "%s: the FULL stage set needs the class row of qact_embed (p2v_plan_set_embed_tap_cls)", who);
  return P2V_OK;
}

// the layout pass: forward_impl's own sequence with no launch made, every stage site listing its record
static int stats_layout(const p2v_plan* plan, int with_linear, int stage_set, std::vector<StatsStage>* out, size_t* total) {
  int rc = stats_stage_set_check(plan, stage_set, "p2v_forward_stats_layout");
  if (rc != P2V_OK) return rc;
  void* const some = reinterpret_cast<void*>(256);      // never dereferenced: nothing is launched
  std::vector<int8_t> cfg(plan->n_layers);
  for (int i = 0; i < plan->n_layers; ++i) cfg[i] = plan->lin_set[bit_index(8)][i] ? 8 : 4;
  StatsCtx sc{nullptr, 0, 0, out};
  DdvCtx ctx{1, nullptr, 0, nullptr, with_linear ? reinterpret_cast<float*>(some) : nullptr, 0};
  ctx.scratch = (stage_set & P2V_DDV_STAGES_FULL) ? reinterpret_cast<float*>(some) : nullptr;
  ctx.attn = (stage_set & P2V_DDV_STAGES_ATTN) ? reinterpret_cast<int8_t*>(some) : nullptr;
  ctx.stats = &sc;
  FwdOpts o;
  o.images = reinterpret_cast<const float*>(some); o.ddv = &ctx; o.dry = true;
  rc = forward_impl(const_cast<p2v_plan*>(plan), 1, cfg.data(), plan->n_layers, reinterpret_cast<float*>(some), some, (size_t)-1, nullptr, o);
  if (rc == P2V_OK && total) *total = sc.off;
  return rc;
}

size_t p2v_forward_stats_bytes(const p2v_plan* plan, int with_linear, int stage_set) {
  std::vector<StatsStage> st;
  size_t total = 0;
  return stats_layout(plan, with_linear, stage_set, &st, &total) == P2V_OK ? total : 0;
}

int p2v_forward_stats_layout(const p2v_plan* plan, int with_linear, int stage_set, int max_stages, long long* offsets, int32_t* cols,
                             int32_t* kinds, const float** scales) {
  std::vector<StatsStage> st;
  const int rc = stats_layout(plan, with_linear, stage_set, &st, nullptr);
  if (rc != P2V_OK) return rc;
  for (int k = 0; k < (int)st.size() && k < max_stages; ++k) {
    if (offsets) offsets[k] = (long long)st[k].off;
    if (cols) cols[k] = st[k].cols;
    if (kinds) kinds[k] = st[k].kind;
    if (scales) scales[k] = st[k].scale;
  }
  return (int)st.size();
}

int p2v_forward_stats(p2v_plan* plan, const float* images, int batch, const int8_t* bit_config, int n_cfg, float* logits, void* ws,
                      size_t ws_bytes, int with_linear, int stage_set, float* tap_scratch, size_t tap_scratch_bytes, int8_t* attn_scratch,
                      size_t attn_scratch_bytes, void* stats, size_t stats_bytes, void* stream) {
  if (!plan || !stats || !ws) return fail(P2V_E_ARG, "p2v_forward_stats: null argument");
  int rc = stats_stage_set_check(plan, stage_set, "p2v_forward_stats");
  if (rc != P2V_OK) return rc;
  const bool full = stage_set & P2V_DDV_STAGES_FULL, attn = stage_set & P2V_DDV_STAGES_ATTN;
  if (batch <= 0 || batch > (1 << 29)) return fail(P2V_E_SHAPE, "p2v_forward_stats: batch = %d", batch);
  if ((uintptr_t)ws % 256) return fail(P2V_E_ARG, "p2v_forward_stats: the workspace must be 256-byte aligned");
  if ((uintptr_t)stats % 16) return fail(P2V_E_ARG, "p2v_forward_stats: the records must be 16-byte aligned");
  const int n = (batch + 1) / 2;                        // the scratch sizes are the DDV call's, which counts pairs of images
  if (full && !tap_scratch)
    return fail(P2V_E_WORKSPACE, "p2v_forward_stats: the FULL stage set needs tap_scratch (%zu bytes) whatever with_linear says", p2v_ddv_tap_scratch_bytes(plan, n));
  if (with_linear || full) {
    if (!tap_scratch) return fail(P2V_E_ARG, "p2v_forward_stats: with_linear needs tap_scratch");
    if ((uintptr_t)tap_scratch % 16) return fail(P2V_E_ARG, "p2v_forward_stats: tap_scratch must be 16-byte aligned");
    if (tap_scratch_bytes < p2v_ddv_tap_scratch_bytes(plan, n))
      return fail(P2V_E_WORKSPACE, "p2v_forward_stats: tap_scratch %zu < %zu bytes", tap_scratch_bytes, p2v_ddv_tap_scratch_bytes(plan, n));
  }
  if (attn) {
    const size_t need = p2v_ddv_attn_scratch_bytes(plan, n);
    if (!attn_scratch) return fail(P2V_E_ARG, "p2v_forward_stats: P2V_DDV_STAGES_ATTN needs attn_scratch (%zu bytes)", need);
    if ((uintptr_t)attn_scratch % 16) return fail(P2V_E_ARG, "p2v_forward_stats: attn_scratch must be 16-byte aligned");
    if (attn_scratch_bytes < need) return fail(P2V_E_WORKSPACE, "p2v_forward_stats: attn_scratch %zu < %zu bytes", attn_scratch_bytes, need);
  }
  StatsCtx sc{reinterpret_cast<char*>(stats), stats_bytes, 0, nullptr};
  DdvCtx ctx{batch, nullptr, 0, nullptr, with_linear ? tap_scratch : nullptr, 0};
  ctx.scratch = full ? tap_scratch : nullptr;
  ctx.attn = attn ? attn_scratch : nullptr;
  ctx.stats = &sc;
  std::vector<float*> taps;
  if (with_linear) {
    taps.assign(plan->n_layers, tap_scratch);      // every linear output goes through the one buffer; the patch embedding is no stage
    taps[0] = nullptr;
  }
  FwdOpts o;
  o.images = images; o.ddv = &ctx; o.lin_tap = with_linear ? taps.data() : nullptr;
  return forward_impl(plan, batch, bit_config, n_cfg, logits, ws, ws_bytes, stream, o);
}

// ---- stage Grams (p2vit_gram.hip; fp32 stages: the partial and reduce launches of p2vit_cka.hip) ------------------------------------------
// aligned: the public rule (base and shift 16-byte aligned); the forward's own stages pass false and the kernels read what is unaligned with
// scalar loads
static int gram_check(const p2v_gram_layer& a, int n, bool aligned, const char* what, int l) {
  if (n < 1 || n > P2V_GRAM_MAX_N) return fail(P2V_E_SHAPE, "%s: n = %d images, the kernels take 1 ... %d", what, n, P2V_GRAM_MAX_N);
  if (!a.base) return fail(P2V_E_ARG, "%s: layer %d has a null base", what, l);
  if (a.dtype != P2V_GRAM_I8 && a.dtype != P2V_GRAM_F32) return fail(P2V_E_ARG, "%s: layer %d: dtype %d (0 = int8, 1 = fp32)", what, l, a.dtype);
  if (a.rows < 1 || a.cols < 1) return fail(P2V_E_SHAPE, "%s: layer %d: %d rows x %d cols", what, l, a.rows, a.cols);
  if (a.row_stride < a.cols) return fail(P2V_E_ARG, "%s: layer %d: row_stride %lld < cols %d", what, l, a.row_stride, a.cols);
  if (a.sample_stride < 0) return fail(P2V_E_ARG, "%s: layer %d: negative sample_stride %lld", what, l, a.sample_stride);
  if (a.shift && a.dtype != P2V_GRAM_I8) return fail(P2V_E_ARG, "%s: layer %d: the shift bytes go with int8 codes", what, l);
  if (aligned && ((uintptr_t)a.base % 16 || (uintptr_t)a.shift % 16))
    return fail(P2V_E_ARG, "%s: layer %d: base and shift must be 16-byte aligned", what, l);
  if (a.dtype == P2V_GRAM_F32 && (uintptr_t)a.base % 4) return fail(P2V_E_ARG, "%s: layer %d: the plane is not aligned to its element", what, l);
  if ((long long)a.rows * a.cols >= (1LL << 31))
    return fail(P2V_E_UNSUPPORTED, "%s: layer %d: %d x %d elements per sample (at most 2^31 - 1)", what, l, a.rows, a.cols);
  if (a.dtype == P2V_GRAM_F32 && a.rows > 1 && a.row_stride != a.cols)
    return fail(P2V_E_UNSUPPORTED, "%s: layer %d: an fp32 stage needs dense rows (row_stride %lld, cols %d)", what, l, a.row_stride, a.cols);
  if (a.dtype == P2V_GRAM_F32 && a.sample_stride < (long long)a.rows * a.cols && n > 1)
    return fail(P2V_E_ARG, "%s: layer %d: sample_stride %lld < rows * cols", what, l, a.sample_stride);
  if (p2v_gram_items(p2v_gram_desc(a), n) >= (1LL << 31)) return fail(P2V_E_UNSUPPORTED, "%s: layer %d: too many partial tiles", what, l);
  return P2V_OK;
}
static p2v_cka_layer gram_as_cka(const p2v_gram_layer& a) {
  return p2v_cka_layer{reinterpret_cast<const float*>(a.base), nullptr, (long long)a.rows * a.cols, a.sample_stride, 0};
}
// the partials of one layer, a multiple of 256 bytes (the layers of one call run one after the other on one stream and share them)
static size_t gram_ws_bytes(const p2v_gram_layer& a, int n) {
  if (a.dtype == P2V_GRAM_F32) {
    const p2v_cka_layer c = gram_as_cka(a);
    return (p2v_cka_layout(&c, 1, n, nullptr).g64_off + 255) / 256 * 256;       // descriptor and chunk partials; the fp64 Gram goes to the output
  }
  return (size_t)p2v_gram_items(p2v_gram_desc(a), n) * 1024 * sizeof(long long);
}
static int gram_launch(const p2v_gram_layer& a, int n, double* G, void* ws, hipStream_t st) {
  if (a.dtype == P2V_GRAM_F32) {
    const p2v_cka_layer c = gram_as_cka(a);
    std::vector<CkaDesc> descs;
    const CkaLayout w = p2v_cka_layout(&c, 1, n, &descs);
    return p2v_launch_cka_raw(descs[0], w, n, G, ws, st);
  }
  return p2v_launch_gram_i8(p2v_gram_desc(a), n, reinterpret_cast<long long*>(ws), G, st);
}

size_t p2v_code_grams_workspace_bytes(const p2v_gram_layer* layers, int n_layers, int n) {
  if (!layers || n_layers <= 0) return 0;
  size_t need = 0;
  for (int l = 0; l < n_layers; ++l) {
    if (gram_check(layers[l], n, true, "p2v_code_grams_workspace_bytes", l) != P2V_OK) return 0;
    const size_t b = gram_ws_bytes(layers[l], n);
    need = b > need ? b : need;
  }
  return need;
}

int p2v_code_grams(const p2v_gram_layer* layers, int n_layers, int n, double* grams, void* ws, size_t ws_bytes, void* stream) {
  if (!layers || n_layers <= 0) return fail(P2V_E_ARG, "p2v_code_grams: no layers");
  if (!grams || !ws) return fail(P2V_E_ARG, "p2v_code_grams: null grams / workspace");
  if ((uintptr_t)grams % 8) return fail(P2V_E_ARG, "p2v_code_grams: grams must be 8-byte aligned");
  if ((uintptr_t)ws % 256) return fail(P2V_E_ARG, "p2v_code_grams: the workspace must be 256-byte aligned");
  size_t need = 0;
  for (int l = 0; l < n_layers; ++l) {
    const int rc = gram_check(layers[l], n, true, "p2v_code_grams", l);
    if (rc != P2V_OK) return rc;
    const size_t b = gram_ws_bytes(layers[l], n);
    need = b > need ? b : need;
  }
  if (ws_bytes < need) return fail(P2V_E_WORKSPACE, "p2v_code_grams: workspace %zu < %zu bytes", ws_bytes, need);
  // (only an fp32 layer uploads a descriptor; one rule for the entry point whatever its layers hold)
  if (const int cap = refuse_capture("p2v_code_grams", "uploads the descriptor of an fp32 layer from host memory that does not outlive it", stream)) return cap;
  for (int l = 0; l < n_layers; ++l) {
    const int rc = launch_rc(gram_launch(layers[l], n, grams + (size_t)l * n * n, ws, (hipStream_t)stream), "code_grams");
    if (rc != P2V_OK) return rc;
  }
  return P2V_OK;
}

int p2v_cka_centre(const double* raw, long long pitch, long long layer_stride, int n_layers, int n, float* grams, void* stream) {
  if (!raw || !grams || n_layers <= 0) return fail(P2V_E_ARG, "p2v_cka_centre: null gram or no layers");
  if (n < P2V_CKA_MIN_N || n > P2V_GRAM_MAX_N) return fail(P2V_E_SHAPE, "p2v_cka_centre: n = %d images, the kernel takes %d ... %d", n, P2V_CKA_MIN_N, P2V_GRAM_MAX_N);
  if (pitch < n || layer_stride < 0) return fail(P2V_E_ARG, "p2v_cka_centre: pitch %lld < n = %d, or a negative layer stride", pitch, n);
  if ((uintptr_t)raw % 8 || (uintptr_t)grams % 4) return fail(P2V_E_ARG, "p2v_cka_centre: misaligned gram");
  return launch_rc(p2v_launch_gram_centre(raw, pitch, layer_stride, n_layers, n, grams, (hipStream_t)stream), "cka_centre");
}

int p2v_plan_prepare_grams(p2v_plan* plan) {
  if (!plan) return fail(P2V_E_ARG, "p2v_plan_prepare_grams: null plan");
  if (!plan->embed_set) return fail(P2V_E_STATE, "p2v_plan_prepare_grams: plan incomplete (embed)");
  for (int i = 0; i < plan->d.depth; ++i)
    if (!plan->block_set[i]) return fail(P2V_E_STATE, "p2v_plan_prepare_grams: plan incomplete (block %d)", i);
  const int D = plan->d.embed_dim, Dp = round_up(D, 16);
  std::vector<const float*> vecs{plan->embed_epi.s_next};
  for (const p2v_block& b : plan->blocks) {
    vecs.push_back(b.proj_epi.s_mid); vecs.push_back(b.proj_epi.s_next);
    vecs.push_back(b.fc2_epi.s_mid); vecs.push_back(b.fc2_epi.s_next);
  }
  for (const float* v : vecs)
    if (!v) return fail(P2V_E_STATE, "p2v_plan_prepare_grams: a stage of the plan has no per-channel scales");
  OwnerDevice dev(vecs[0]);
  if (!dev.ok()) return fail(P2V_E_ARG, "p2v_plan_prepare_grams: cannot locate the device of the plan's scales");
  if (hipDeviceSynchronize() != hipSuccess) return fail(P2V_E_LAUNCH, "p2v_plan_prepare_grams: %s", hipGetErrorString(hipGetLastError()));
  std::vector<float> host(D);
  std::vector<uint8_t> bytes(vecs.size() * (size_t)Dp, 0);
  std::vector<p2v_plan::GramScale> found;
  for (size_t v = 0; v < vecs.size(); ++v) {
    if (hipMemcpy(host.data(), vecs[v], (size_t)D * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
      return fail(P2V_E_LAUNCH, "p2v_plan_prepare_grams: %s", hipGetErrorString(hipGetLastError()));
    float lo = host[0];
    for (int c = 1; c < D; ++c) lo = host[c] < lo ? host[c] : lo;
    if (!(lo > 0.f) || !(lo < INFINITY)) return fail(P2V_E_UNSUPPORTED, "p2v_plan_prepare_grams: scale vector %zu holds %g", v, lo);
    for (int c = 0; c < D; ++c) {
      const float q = host[c] / lo;
      const int m = q == 1.f ? 0 : q == 2.f ? 1 : q == 4.f ? 2 : q == 8.f ? 3 : -1;
      if (m < 0 || lo * q != host[c])
        return fail(P2V_E_UNSUPPORTED, "p2v_plan_prepare_grams: scale vector %zu: s[%d] / min s = %g is not 1, 2, 4 or 8", v, c, (double)host[c] / lo);
      bytes[v * Dp + c] = (uint8_t)m;
    }
    found.push_back(p2v_plan::GramScale{vecs[v], nullptr, (double)lo});
  }
  uint8_t* buf = plan->gram_shift_buf;
  if (!buf && hipMalloc(&buf, bytes.size()) != hipSuccess) return fail(P2V_E_LAUNCH, "p2v_plan_prepare_grams: %s", hipGetErrorString(hipGetLastError()));
  plan->gram_shift_buf = buf;
  if (plan->device < 0) plan->device = dev.own;
  if (hipMemcpy(buf, bytes.data(), bytes.size(), hipMemcpyHostToDevice) != hipSuccess)
    return fail(P2V_E_LAUNCH, "p2v_plan_prepare_grams: %s", hipGetErrorString(hipGetLastError()));
  for (size_t v = 0; v < found.size(); ++v) found[v].shift = buf + v * Dp;
  plan->gram_scales = found;
  plan->grams_ready = true;
  return P2V_OK;
}

static int grams_stage_set_check(const p2v_plan* plan, int stage_set, const char* who) {
  if (!plan) return fail(P2V_E_ARG, "%s: null argument", who);
  if (stage_set >= 0 && stage_set <= (P2V_DDV_STAGES_FULL | P2V_DDV_STAGES_ATTN) && (stage_set & P2V_DDV_STAGES_ATTN))
    return fail(P2V_E_UNSUPPORTED, "%s: P2V_DDV_STAGES_ATTN: the exponent planes of the attention stages are no byte codes", who);
  return stats_stage_set_check(plan, stage_set, who);
}

// the layout pass: forward_impl's own sequence with no launch made, every stage site listing itself
static int grams_layout(const p2v_plan* plan, int with_linear, int stage_set, std::vector<GramStage>* out) {
  int rc = grams_stage_set_check(plan, stage_set, "p2v_forward_grams_layout");
  if (rc != P2V_OK) return rc;
  void* const some = reinterpret_cast<void*>(256);      // never dereferenced: nothing is launched
  std::vector<int8_t> cfg(plan->n_layers);
  for (int i = 0; i < plan->n_layers; ++i) cfg[i] = plan->lin_set[bit_index(8)][i] ? 8 : 4;
  GramsCtx gc{plan, nullptr, nullptr, nullptr, 0, out, {}};
  DdvCtx ctx{1, nullptr, 0, nullptr, with_linear ? reinterpret_cast<float*>(some) : nullptr, 0};
  ctx.scratch = (stage_set & P2V_DDV_STAGES_FULL) ? reinterpret_cast<float*>(some) : nullptr;
  ctx.grams = &gc;
  FwdOpts o;
  o.images = reinterpret_cast<const float*>(some); o.ddv = &ctx; o.dry = true;
  return forward_impl(const_cast<p2v_plan*>(plan), 1, cfg.data(), plan->n_layers, reinterpret_cast<float*>(some), some, (size_t)-1, nullptr, o);
}

int p2v_forward_grams_stage_count(const p2v_plan* plan, int with_linear, int stage_set) {
  const int rc = grams_stage_set_check(plan, stage_set, "p2v_forward_grams_stage_count");
  return rc != P2V_OK ? rc : p2v_ddv_stage_count_ex(plan, with_linear, stage_set);
}

// the partials of the largest stage at `batch` samples (the forward's stages are dense or pitched planes of its own buffers)
static size_t grams_partial_bytes(const std::vector<GramStage>& st, int batch) {
  size_t need = 0;
  for (const GramStage& s : st) {
    const p2v_gram_layer l{reinterpret_cast<const void*>(256), nullptr, (long long)s.rows * s.cols, s.cols, s.rows, s.cols, s.kind};
    const size_t b = gram_ws_bytes(l, batch);
    need = b > need ? b : need;
  }
  return need;
}

size_t p2v_forward_grams_bytes(const p2v_plan* plan, int batch, int with_linear, int stage_set) {
  std::vector<GramStage> st;
  if (batch < 1 || batch > P2V_GRAM_MAX_N || grams_layout(plan, with_linear, stage_set, &st) != P2V_OK) return 0;
  return ws_layout(plan, batch).total + grams_partial_bytes(st, batch);        // (the forward's part is a multiple of 256 bytes)
}

int p2v_forward_grams_layout(const p2v_plan* plan, int with_linear, int stage_set, int max_stages, int32_t* rows, int32_t* cols,
                             int32_t* kinds, const float** scales) {
  std::vector<GramStage> st;
  const int rc = grams_layout(plan, with_linear, stage_set, &st);
  if (rc != P2V_OK) return rc;
  for (int k = 0; k < (int)st.size() && k < max_stages; ++k) {
    if (rows) rows[k] = st[k].rows;
    if (cols) cols[k] = st[k].cols;
    if (kinds) kinds[k] = st[k].kind;
    if (scales) scales[k] = st[k].scale;
  }
  return (int)st.size();
}

int p2v_forward_grams(p2v_plan* plan, const float* images, int batch, const int8_t* bit_config, int n_cfg, float* logits, void* ws,
                      size_t ws_bytes, int with_linear, int stage_set, float* tap_scratch, size_t tap_scratch_bytes, double* grams,
                      size_t grams_bytes, double* units, size_t units_bytes, void* stream) {
  if (!plan || !grams || !units || !ws) return fail(P2V_E_ARG, "p2v_forward_grams: null argument");
  std::vector<GramStage> stages;
  int rc = grams_layout(plan, with_linear, stage_set, &stages);
  if (rc != P2V_OK) return rc;
  if (!plan->grams_ready) return fail(P2V_E_STATE, "p2v_forward_grams: call p2v_plan_prepare_grams on the finished plan first");
  const bool full = stage_set & P2V_DDV_STAGES_FULL;
  if (batch < 1 || batch > P2V_GRAM_MAX_N) return fail(P2V_E_SHAPE, "p2v_forward_grams: batch = %d images, the kernels take 1 ... %d", batch, P2V_GRAM_MAX_N);
  if ((uintptr_t)ws % 256) return fail(P2V_E_ARG, "p2v_forward_grams: the workspace must be 256-byte aligned");
  if ((uintptr_t)grams % 8 || (uintptr_t)units % 8) return fail(P2V_E_ARG, "p2v_forward_grams: grams and units must be 8-byte aligned");
  const size_t K = stages.size();
  if (grams_bytes < K * batch * batch * sizeof(double))
    return fail(P2V_E_WORKSPACE, "p2v_forward_grams: grams %zu < %zu bytes", grams_bytes, K * batch * batch * sizeof(double));
  if (units_bytes < K * sizeof(double)) return fail(P2V_E_WORKSPACE, "p2v_forward_grams: units %zu < %zu bytes", units_bytes, K * sizeof(double));
  const size_t fwd = ws_layout(plan, batch).total, part = grams_partial_bytes(stages, batch);
  if (ws_bytes < fwd + part) return fail(P2V_E_WORKSPACE, "p2v_forward_grams: workspace %zu < %zu bytes", ws_bytes, fwd + part);
  const int n = (batch + 1) / 2;                        // the scratch size is the DDV call's, which counts pairs of images
  if (full && !tap_scratch)
    return fail(P2V_E_WORKSPACE, "p2v_forward_grams: the FULL stage set needs tap_scratch (%zu bytes) whatever with_linear says", p2v_ddv_tap_scratch_bytes(plan, n));
  if (with_linear || full) {
    if (!tap_scratch) return fail(P2V_E_ARG, "p2v_forward_grams: with_linear needs tap_scratch");
    if ((uintptr_t)tap_scratch % 16) return fail(P2V_E_ARG, "p2v_forward_grams: tap_scratch must be 16-byte aligned");
    if (tap_scratch_bytes < p2v_ddv_tap_scratch_bytes(plan, n))
      return fail(P2V_E_WORKSPACE, "p2v_forward_grams: tap_scratch %zu < %zu bytes", tap_scratch_bytes, p2v_ddv_tap_scratch_bytes(plan, n));
  }
  if (const int cap = refuse_capture("p2v_forward_grams", "uploads the stage units and fp32 descriptors from host memory that does not outlive it", stream))
    return cap;
  GramsCtx gc{plan, grams, units, reinterpret_cast<char*>(ws) + fwd, part, nullptr, {}};
  gc.host_units.reserve(K);
  DdvCtx ctx{batch, nullptr, 0, nullptr, with_linear ? tap_scratch : nullptr, 0};
  ctx.scratch = full ? tap_scratch : nullptr;
  ctx.grams = &gc;
  std::vector<float*> taps;
  if (with_linear) {
    taps.assign(plan->n_layers, tap_scratch);      // every linear output goes through the one buffer; the patch embedding is no stage
    taps[0] = nullptr;
  }
  FwdOpts o;
  o.images = images; o.ddv = &ctx; o.lin_tap = with_linear ? taps.data() : nullptr;
  rc = forward_impl(plan, batch, bit_config, n_cfg, logits, ws, fwd, stream, o);
  if (rc != P2V_OK) return rc;
  if (gc.host_units.size() != K) return fail(P2V_E_STATE, "p2v_forward_grams: %zu stages ran, the layout lists %zu", gc.host_units.size(), K);
  // pageable source on a stream that is NOT capturing (refused above): the runtime stages it before returning, so the host vector may go
  // away afterwards.  Recorded into a graph the copy node would keep the host pointer and every replay would read freed memory
  if (hipMemcpyAsync(units, gc.host_units.data(), K * sizeof(double), hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess)
    return fail(P2V_E_LAUNCH, "p2v_forward_grams: %s", hipGetErrorString(hipGetLastError()));
  return P2V_OK;
}
