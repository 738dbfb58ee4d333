// Host-side plans and kernel-launch drivers: one v4l_net = one reference network (state MLP, NatureCNN fuse
// net or LocoTransformer), one v4l_trainer = the PPO minibatch update over (pf, vf, target_pf).
#pragma once
#include <string>
#include <vector>

#include "../../include/v4l_hip.h"
#include "elem.h"
#include "gemm.h"

namespace v4l { struct RowsChain; struct FbLoss; }

namespace v4l {

struct ParamInfo {
  std::string name;
  int ndim;
  int64_t shape[4];
  int64_t numel;
  int64_t goff;  // offset in the flat grad / moment buffers
};

struct Lin {         // nn.Linear (or the 1x1 up-conv): y = x W^T + b, W [N][K]
  int w = -1, b = -1;
  int N = 0, K = 0;
  int Np = 0, Kp = 0;     // forward pack [Np][Kp]
  int64_t pk = 0;
  int Rt = 0, Ct = 0;     // transposed pack [Rt = pad16(K)][Ct = pad64(N)] for the data-grad
  int64_t pkt = 0;
  int64_t pkf = -1;       // fragment-order pack [Np/16][Kp/32][64 lanes][8] (rollout kernels, gemm_nt_deep_kernel), -1: none
  int64_t pkft = -1;      // the same of W^T: [Rt/16][Ct/32][64][8] (data-grads through gemm_nt_deep_kernel), -1: none
  int64_t pkp = -1, pkpt = -1;  // k-permuted fragment-order packs of W / W^T (wave-per-sample layer kernels, csrc/wps.h), -1: none
  int64_t pko = -1, pkto = -1;  // vision-only Transformer, first head layer: [N][128] / [128][N] row-major packs with the 64
                                // real K entries at offset 64 (the pooled operand's second half), -1: none
  int cin = 0, taps = 0;  // > 0: input is an NHWC flatten, packed k = tap*cin + c  (PyTorch k = c*taps + tap)
  bool need_dgrad = true;
  std::string tag_fwd, tag_wgrad, tag_dgrad;  // profiler labels
};

struct Conv {        // nn.Conv2d, square kernel, no padding. Activations NHWC, conv1 reads the CHW depth stack.
  int w = -1, b = -1;
  int Cin = 0, Cout = 0, KH = 0, stride = 0, IH = 0, OH = 0;
  int K = 0, Kp = 0, Np = 0;
  int64_t pk = 0;
  int64_t pkf = -1;       // fragment-order pack (rollout_encoder2_kernel), -1: none
  bool chw = false;       // conv1
  int ncls = 0;           // stride*stride parity classes of the gather-form data-grad
  int Kd = 0, Kdp = 0, Rd = 0;
  int64_t pkd[4] = {0, 0, 0, 0};
};

struct LNp { int g = -1, b = -1; };
struct TLayer { Lin inproj, outproj, ff1, ff2; LNp ln1, ln2; };

// fused layer kernels keep xin (copy of the layer input), ctx, x1, f in the contraction type T inside these fp32-sized slots
struct LayerWs { int64_t qkv, P, ctx, xh1, rs1, x1, f, xh2, rs2, xin; };
// backward: every layer keeps its own gradient tensors alive until the grouped weight-grad launch at the end
struct LayerBw { int64_t dz2, df, dx1, dz1, dctx, dqkv; };
struct Layout {
  int n = 0;
  int64_t c1 = 0, c2 = 0, c3 = 0;
  std::vector<int64_t> eh;       // encoder MLP activations
  int64_t vis = 0;               // CNN: concat buffer [n][visual_dim + enc_last]
  std::vector<int64_t> x;        // LOCO: token tensors x[0..L]
  int64_t xfin = 0, xhF = 0, rsF = 0, dxfin = 0;    // pytorch_encoder: the final LayerNorm's output, xhat / rstd, grad w.r.t. its output
  int64_t x0raw = 0, xh0 = 0, rs0 = 0, dx0raw = 0;  // token_norm: the encoder's tokens (x[0] = their LayerNorm), xhat / rstd, grad w.r.t. them
  std::vector<LayerWs> lw;
  int64_t ytmp = 0;              // [R][64] sub-layer output before add+LN
  int64_t pooled = 0;
  std::vector<int64_t> hh;       // head hidden activations
  int64_t out = 0, dout = 0;     // [n][OUT_LD]
  // backward: one buffer per gradient tensor (nothing is overwritten before the deferred weight-grads ran)
  std::vector<int64_t> dhh;      // grad w.r.t. head hidden pre-activations
  std::vector<int64_t> deh;      // grad w.r.t. encoder-MLP hidden pre-activations
  std::vector<LayerBw> lb;
  std::vector<int64_t> dxl;      // LOCO: grad w.r.t. x[l], l = 0..L
  int64_t dhc = 0;               // [n][maxwidth] hand-off between two stacks (head -> encoder / concat)
  int64_t dpool = 0, dc3 = 0, dc2 = 0, dc1 = 0;
  std::vector<int64_t> wps_wg, wps_tk;  // per layer: fragment-order weight-grad operand blocks of the wave-per-sample kernels
  int64_t slab = 0;              // weight-grad partial slabs
  int64_t total = 0;
};

// The kernels that run the Transformer layers of a training pass (v4l_net::layer_route), forward and backward alike
enum class LayerFamily {
  NONE,             // state MLP / NatureCNN nets: no Transformer layers
  WPS_PLAIN,        // the shipped LocoTransformer (mean or max pooling): wps_layer_fwd_kernel / wps_layer_bwd_kernel, or the two
                    // as wps_layer_fb_kernel when the trainer hands the loss over (fb_allowed)
  WPS_VIS,          // vision-only net: the same pair, native 16-token instantiation (VIS = 2)
  WPS_VIS17,        // vision-only net, V4L_VIS17 / V4L_LAYER_TAPS: the 17-row instantiation (dummy row 0)
  WPS_OPT,          // token_norm / use_pytorch_encoder / another proprio MLP: the wave-per-sample pair (MODE 1..3) between
                    // layer-by-layer launches (token_ln; the final norm + pooling + heads; the encoder-side data-grads)
  WPS_OPT_VIS,      // the same for the vision-only net (VIS = 2 over 17-row slots)
  BLOCK_STACK,      // infer_layer_kernel<.., NL = 2>; bwd_layer_kernel<.., NL = 2> (NL = 1 twice unless tail_in)
  BLOCK_PER_LAYER,  // infer_layer_kernel / bwd_layer_kernel, NL = 1: one launch per layer, heads / tail riding on the outer ones
  LAYER_BY_LAYER,   // GEMM + attention + LayerNorm launches (lin_fwd, attn_fwd_kernel, add_ln_fwd_kernel and their backwards)
};
struct LayerRoute {
  LayerFamily family = LayerFamily::NONE;
  bool heads_in = false;  // the pooled heads run inside the layers' launch (else: final norm / pooling / head chain launches)
  bool tail_in = false;   // the encoder-side data-grads (proprio MLP + projector, up-conv) come out of the layers' launch
  bool rows17 = false;    // vision-only net on the wave-per-sample kernels: its 16 tokens sit in rows 1..16 of 17-row slots
  bool fb_allowed = false;         // the trainer may hand the loss over for the fused forward-loss-backward launch (V4L_NO_FB: never)
  bool heads_ext_allowed = false;  // ... may run the policy's pooled-heads data-grad chain beside the loss statistics
  bool heads_ext_critic = false;   // ... and the critic's (V4L_WPS_HEAD_EXT_CRITIC)
  // diagnostic switches, read once per pass
  bool taps = false;      // V4L_LAYER_TAPS: the kernels also write every intermediate (tests)
  bool stack_ok = true;   // !V4L_NO_LAYER_STACK
  bool tok0_in = false;   // V4L_WPS_TOK0_IN: the proprio branch's data-grad chain stays inside the backward launch
  int par_wgrad = 2;      // V4L_PAR_WGRAD: schedule of the weight-grad section (backward_t)
  bool wps() const { return family >= LayerFamily::WPS_PLAIN && family <= LayerFamily::WPS_OPT_VIS; }
  bool opt() const { return family == LayerFamily::WPS_OPT || family == LayerFamily::WPS_OPT_VIS; }
  bool block() const { return family == LayerFamily::BLOCK_STACK || family == LayerFamily::BLOCK_PER_LAYER; }
};

}  // namespace v4l

struct v4l_net {
  v4l_net_cfg cfg;
  int Sp = 0;
  int ntok = v4l::NTOK;  // tokens per sample: 17 (LocoTransformer), 16 (vision-only Transformer)
  // c1 / c2 of the training forward in the operand type (round 5): asked for by v4l_net_forward(train = 1) — the trainer's and
  // the tests' forward / backward pairs —, granted by forward_t when the persistent training encoder writes them and the fused
  // conv backward will read them (bf16, shipped conv geometry, no test taps), remembered for the backward of the same pass
  bool want_acts16 = false;
  const float* acts16_c1 = nullptr;  // the c1 slot (= the workspace) whose c1 / c2 currently hold the operand type; null: none
  bool vis_only() const { return cfg.kind == V4L_NET_CNN_VIS || cfg.kind == V4L_NET_LOCO_VIS; }
  bool is_tf() const { return cfg.kind == V4L_NET_LOCO || cfg.kind == V4L_NET_LOCO_VIS; }
  // GaussianContPolicy (continuous_policy.py:222-236): the head's last layer is [mean | raw log sigma], out_dim = 2 A columns
  bool sd() const { return cfg.has_logstd == V4L_LOGSTD_HEAD; }
  // action dimensions A of a policy: the head's width, or half of it where the other half is the per-row log sigma
  // CategoricalDisPolicy (policies/discrete_policies.py:127-172; v4l_net_set_categorical): a has_logstd = 0 state-MLP net whose
  // K = out_dim head columns are the logits of a policy over K actions. Not a cfg field: v4l_net_cfg is frozen
  bool categorical = false;
  bool cat() const { return categorical; }
  // true for every net a trainer / an actor takes as its policy
  bool is_policy() const { return cfg.has_logstd != V4L_LOGSTD_NONE || categorical; }
  int act_dim() const { return cat() ? 1 : sd() ? cfg.out_dim / 2 : cfg.out_dim; }
  std::vector<v4l::ParamInfo> params;
  int64_t total_params = 0;
  // layers
  v4l::Conv conv[3];
  v4l::Lin upconv, proj;            // LOCO: depth_up_conv, state_projector ; CNN: proj = visual_projector
  std::vector<v4l::Lin> enc;        // encoder.base / Net.base MLP
  std::vector<v4l::TLayer> layers;
  v4l::LNp fin_ln;                  // cfg.pytorch_encoder: nn.TransformerEncoder's final norm
  v4l::LNp tok_ln, stok_ln;         // cfg.token_norm: token_ln (applied to every token), state_token_ln (a parameter nobody uses)
  std::vector<v4l::Lin> head;       // append fcs + last
  int logstd = -1;
  int64_t packed_elems = 0;
  std::vector<v4l::PackDesc> packs;  // src filled at bind
  std::vector<int> pack_param;       // param index per desc
  int64_t pack_blocks = 0;
  // binding
  std::vector<float*> p;             // device pointers per param
  void* packed = nullptr;
  v4l::PackDesc* d_packs = nullptr;
  v4l::ParamSeg* d_segs = nullptr;
  v4l::RedDesc* d_red = nullptr;
  float* d_sq = nullptr;             // sum of squares of what each wgrad_reduce block wrote (the gradient norm's partials)
  int64_t sq_cap() const { return total_params / 64 + 2 * MAX_RED + 64; }
  int red_blocks = 0;                // blocks of the last wgrad_reduce launch (0: no partials available)
  const float* red_grads = nullptr;  // the gradient buffer that launch wrote: the partials describe THIS buffer only
  static constexpr int MAX_RED = 96;
  static constexpr int MAX_TNP = 64;
  v4l::TnProb* d_tnp = nullptr;
  static constexpr int MAX_WIDE = 16;
  v4l::TnWide* d_wide = nullptr;
  std::vector<v4l::TnWide> wide, wide_cached;  // whole-output weight-grad problems of the fused transformer layers
  double wide_flops = 0;
  double tnp_flops = 0;
  std::vector<v4l::TnProb> tnp, tnp_cached;   // deferred dense weight-grad problems of the current / last backward
  std::vector<v4l::RedDesc> red, red_cached;  // weight-grad reduce descriptors of the current / last backward
  int64_t slab_cap = 0;
  float grad_unscale = 1.f;          // 1 / the gradient scale of the backward pass in flight (V4L_F16; 1 otherwise)
  float grad_scale_next = 0.f;       // v4l_net_set_grad_scale: the next backward pass's scale (0: the rule of v4l_net_grad_scale)
  int64_t seg_blocks = 0;
  bool bound = false;
  int gen = 0;  // bind generation: bumped by every v4l_net_bind; captured graphs of trainers / actors are keyed on it
  // auxiliary stream + fork/join events for sibling-kernel concurrency (created at bind; null = serial)
  hipStream_t aux = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipStream_t aux2 = nullptr;  // third branch of the weight-grad section (V4L_PAR_WGRAD=3)
  hipEvent_t ev_fork2 = nullptr, ev_join2 = nullptr;

  int build();
  v4l::Layout layout(int n) const;
  int64_t table_bytes() const;
  int64_t slab_floats(int n) const;
  // enc_ws != null: reuse the encoder output another net (same encoder parameters and shapes) left in ITS workspace
  // stage: 0 = whole net, 1 = encoder only (up to the token / concat tensor), 2 = trunk + head only
  template <typename T> int forward_t(const float* state, const T* image, const int* rowidx, int n, float* ws, hipStream_t s,
                                      const float* enc_ws = nullptr, int stage = 0);
  // Which kernels run the Transformer layers of a training pass: decided here, once, for forward_t, backward_t, heads_ext and
  // the trainer alike (the wave-per-sample forward saves only the layers' input rows, which only the wave-per-sample backward
  // can start from). Reads cfg, the pack offsets and the diagnostic switches — per call, nothing is kept: tests switch them
  // between two passes of one process. whole_pass = false: a forward over another net's encoder output, or over one stage
  // only, stays off the vision / option routes (as under V4L_NO_WPS_LAYERS).
  v4l::LayerRoute layer_route(bool whole_pass = true) const;
  bool wps_tail_shape() const;  // the proprio MLP the wave-per-sample backward continues into (256-256)
  // round 4: the pooled heads' data-grads ran beside the loss statistics (heads_ext() handed the trainer their operands) for
  // the backward pass over (heads_ext_ws, heads_ext_n) that follows; backward_t consumes the mark
  float* heads_ext_ws = nullptr;
  int heads_ext_n = 0;
  int heads_ext(float* ws, int n, v4l::RowsChain* out, bool critic = false);
  // round 6: the trainer handed over the loss of the pass (rows, scalars, where the statistics go) — backward_t then runs the
  // layers' forward, the loss rows and the backward as ONE launch (csrc/wps_fb.h) over a workspace whose forward stopped behind
  // the encoder (forward_t stage 1); backward_t consumes the mark. Only for a net whose layer_route().fb_allowed says so.
  const v4l::FbLoss* fb_loss = nullptr;
  template <typename T> int backward_t(const float* state, const T* image, const int* rowidx, int n, float* ws, float* grads, hipStream_t s);
};

struct v4l_actor {
  v4l_net *pf = nullptr, *vf = nullptr;
  hipStream_t aux = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int E = 0;
  float* ws = nullptr;
  v4l::ActCtl* ctl = nullptr;
  int* rowidx = nullptr;
  hipGraphExec_t gexec = nullptr;
  const void* key[16] = {};
  bool warm = false, bound = false;
  long long t_host = -1;  // the env step index as the host counts it (v4l_actor_seek sets it, eager steps advance it); -1: unknown
  // host mirror of ActCtl::seq (launches of rollout_dense_kernel so far; v4l_actor_bind zeroes both): eager launches pass it as
  // an argument. dense_in_graph: the captured step contains that kernel, so every replay advances the device's count too.
  unsigned dense_seq = 0;
  bool dense_in_graph = false;
};

struct GraphKey { v4l_rollout ro; v4l_ppo_hyper hp; int n; int gen[3]; };
// everything a captured V-MPO update bakes into its nodes beyond GraphKey: the V-MPO block (its owner moves it when the
// minibatch grows), the V-MPO record array and the stored v4l_vmpo_hyper (compared bytewise: zero the key first)
struct VmpoGraphKey { GraphKey base; const void* block; const float* vstats_all; v4l_vmpo_hyper vhp; };
// a captured A2C update bakes in GraphKey's fields and the A2C record array (compared bytewise: zero the key first)
struct A2cGraphKey { GraphKey base; const float* astats_all; };

struct v4l_trainer {
  v4l_net *pf = nullptr, *vf = nullptr, *tpf = nullptr;
  float *g_pf = nullptr, *m_pf = nullptr, *v_pf = nullptr, *g_vf = nullptr, *m_vf = nullptr, *v_vf = nullptr;
  float* ws = nullptr;
  int64_t ws_floats = 0;
  // device control block + per-update staging (caller-allocated, v4l_trainer_ctl_bytes)
  v4l::UpdCtl* ctl = nullptr;
  float* stats_cur = nullptr;
  int* rowidx_cur = nullptr;
  float* norm_part = nullptr;
  int n_max = 0;
  const int* rowidx_all = nullptr;
  float* stats_all = nullptr;
  int* skip_all = nullptr;  // [U][2] skipped-step flags of a guarded run (v4l_trainer_begin_guarded); null: the guard is off
  hipStream_t aux = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // hipGraph of one minibatch update
  GraphKey gkey = {};
  hipGraphExec_t gexec = nullptr;
  hipGraphExec_t gexec_run = nullptr;  // hipGraph of a whole run of updates (v4l_trainer_update_run), gexec_run_count of them
  int gexec_run_count = 0;
  bool warm = false;
  bool bound = false;
  // data parallel: RCCL communicator of this trainer's process group (null: single GPU, or the host drives the exchange)
  void* comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  // V-MPO (v4l_trainer_vmpo_init): the caller's device block [VmpoState | record being filled | selected rows] and the hyper-parameters
  v4l::VmpoState* vmpo = nullptr;
  float* vmpo_stats_cur = nullptr;
  int* vmpo_sel = nullptr;
  int vmpo_n_max = 0;
  v4l_vmpo_hyper vmpo_hp = {};
  // hipGraphs of a V-MPO update / of a run of them: a key and handles of their own, never PPO's (v4l_trainer_vmpo_update_next)
  VmpoGraphKey vkey = {};
  hipGraphExec_t vexec = nullptr;
  hipGraphExec_t vexec_run = nullptr;
  int vexec_run_count = 0;
  bool vwarm = false;
  int64_t vmpo_captures = 0, vmpo_replays = 0;  // graphs instantiated / hipGraphLaunch calls (v4l_trainer_vmpo_graph_counts)
  // hipGraphs of an A2C update / of a run of them: a key and handles of their own, never PPO's or V-MPO's (v4l_trainer_a2c_update_next)
  A2cGraphKey akey = {};
  hipGraphExec_t aexec = nullptr;
  hipGraphExec_t aexec_run = nullptr;
  int aexec_run_count = 0;
  bool awarm = false;
  int64_t a2c_captures = 0, a2c_replays = 0;  // graphs instantiated / hipGraphLaunch calls (v4l_trainer_a2c_graph_counts)
  // hipGraphs of a REINFORCE update / of a run of them: the same key type (GraphKey + the record array), a key and handles of
  // their own (v4l_trainer_reinforce_update_next)
  A2cGraphKey rkey = {};
  hipGraphExec_t rexec = nullptr;
  hipGraphExec_t rexec_run = nullptr;
  int rexec_run_count = 0;
  bool rwarm = false;
  int64_t reinforce_captures = 0, reinforce_replays = 0;  // (v4l_trainer_reinforce_graph_counts)
  // the KL early stop (v4l_trainer_kl_stop): [U][2] floats {approx_kl, latch} per update, null: disarmed; kl_thresh = 1.5 * target_kl.
  // Armed updates run through entry points of their own (v4l_trainer_kl_update_next / _update_run) with a key (GraphKey + the KL
  // array) and handles of their own; PPO's entry points and graphs are as they were
  float* kl_all = nullptr;
  double kl_thresh = 0.0;
  A2cGraphKey kkey = {};
  hipGraphExec_t kexec = nullptr;
  hipGraphExec_t kexec_run = nullptr;
  int kexec_run_count = 0;
  bool kwarm = false;
  int64_t kl_captures = 0, kl_replays = 0;
  // the KL-adaptive learning rates (v4l_trainer_kl_adapt): [U][4] floats {approx_kl, decision, lr_pf, lr_vf} per update, null:
  // disarmed; ad_num = {desired_kl, factor, lr_min, lr_max}, baked into the captured kl_adapt launches. Entry points
  // (v4l_trainer_kl_adapt_update_next / _update_run), key (GraphKey + the array) and handles of their own, like the early stop's
  float* ad_all = nullptr;
  double ad_num[4] = {0.0, 0.0, 0.0, 0.0};
  A2cGraphKey dkey = {};
  hipGraphExec_t dexec = nullptr;
  hipGraphExec_t dexec_run = nullptr;
  int dexec_run_count = 0;
  bool dwarm = false;
  int64_t ad_captures = 0, ad_replays = 0;
};
