// Non-GEMM kernels of the PPO hot path: observation ingest, 17-token single-head attention (fwd/bwd),
// residual + LayerNorm (fwd/bwd), token pooling, Gaussian-policy head, PPO losses, advantage statistics,
// global-norm + Adam, weight packing and GAE. All fp32 (GAE fp64) on the VALU; one wave = 64 lanes.
#pragma once
#include "common.h"
#include "../../include/v4l_hip.h"

namespace v4l {

constexpr int NTOK = 17;   // 1 proprio token + 4x4 depth patches (torchrl/networks/base.py:544,617-622)
constexpr int TD = 64;     // token_dim (torchrl/networks/base.py:504)
constexpr int OUT_LD = 16; // row stride of head outputs / their grads (A <= V4L_MAX_ACT or 1, zero padded)
constexpr float LOG_SIG_MAX = 2.f, LOG_SIG_MIN = -5.f;  // torchrl/policies/continuous_policy.py:8-9
constexpr float HALF_LOG_2PI = 0.91893853320467274178f;

// --------------------------------------------------------------------------------- ingest
// Splits reference observation rows [n][S + C*H*W] (torchrl/networks/nets.py:997-1000) into the two
// device-resident arrays the kernels read: proprio [slot][Sp] fp32 (zero padded to Sp) and the depth
// stack [slot][C*H*W] in the contraction operand type. One block per row.
template <typename ImgT>
__global__ __launch_bounds__(256) void ingest_kernel(const float* __restrict__ obs, int n, int S, int Sp, int img_elems,
                                                     float* __restrict__ state, ImgT* __restrict__ image, int64_t slot0,
                                                     const long long* __restrict__ step_counter) {
  const int r = blockIdx.x;
  if (r >= n) return;
  if (step_counter != nullptr) slot0 = (int64_t)(*step_counter) * n;  // device-side rollout cursor (actor graph)
  const float* src = obs + (int64_t)r * (S + img_elems);
  float* sdst = state + (slot0 + r) * (int64_t)Sp;
  ImgT* idst = image + (slot0 + r) * (int64_t)img_elems;
  for (int i = threadIdx.x; i < Sp; i += 256) sdst[i] = i < S ? src[i] : 0.f;
  const float* isrc = src + S;
  for (int i = threadIdx.x; i < img_elems; i += 256) idst[i] = Op<ImgT>::from_f32(isrc[i]);
}

// --------------------------------------------------------------------------------- attention
// nn.MultiheadAttention(64, 1 head) core on packed qkv rows [n*17][192] (q|k|v), per sample:
//   P = softmax(q k^T / sqrt(64)),  ctx = P v.   NT tokens per sample: 17 (LocoTransformer) or 16 (vision-only Transformer).          (torch nn/functional.py multi_head_attention_forward;
// built by the reference at torchrl/networks/nets.py:948-955). One wave per sample, 4 samples per block.
constexpr int ATT_LD = TD + 1;  // +1 float: conflict-free both for lane=d and lane=(i,j) access
constexpr int ATT_PLD = 20;

// x as a contraction of compute mode `bf` sees it (0: fp32, 1: bf16, 2: f16 — ModeOf<T>::value)
__device__ __forceinline__ float rbf(float x, int bf) { return bf == 1 ? (float)(__bf16)x : bf == 2 ? (float)(_Float16)x : x; }
template <int NT>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const float* __restrict__ qkv, int n, float* __restrict__ P,
                                                       float* __restrict__ ctx, int bf) {
  // bf: bf16 compute mode — the operands of the two products (q, k; P, v) are rounded to bf16 like the MFMA tiles of the
  // fused kernels round theirs (attn_tile, csrc/infer.h); accumulation, scale and softmax stay fp32
  // one sample per block: the 289 scores and the 17x64 context are spread over all 256 threads (the per-sample
  // dependency chain, not throughput, is what bounds this kernel)
  __shared__ float q[NT * ATT_LD], k[NT * ATT_LD], v[NT * ATT_LD], p[NT * ATT_PLD];
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const float* src = qkv + (int64_t)b * NT * 3 * TD;
  for (int idx = tid; idx < NT * 3 * TD; idx += 256) {
    const int t = idx / (3 * TD), c = idx - t * 3 * TD;
    const int part = c >> 6, d = c & 63;
    (part == 0 ? q : part == 1 ? k : v)[t * ATT_LD + d] = rbf(src[idx], bf);
  }
  __syncthreads();
  for (int pr = tid; pr < NT * NT; pr += 256) {
    const int i = pr / NT, j = pr - i * NT;
    float s = 0.f;
#pragma unroll 16
    for (int d = 0; d < TD; ++d) s = fmaf(q[i * ATT_LD + d], k[j * ATT_LD + d], s);
    p[i * ATT_PLD + j] = s * 0.125f;
  }
  __syncthreads();
  if (tid < NT) {
    float mx = -INFINITY;
    for (int j = 0; j < NT; ++j) mx = fmaxf(mx, p[tid * ATT_PLD + j]);
    float e[NT], sum = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j) { e[j] = expf(p[tid * ATT_PLD + j] - mx); sum += e[j]; }
    const float inv = 1.f / sum;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const float pv = e[j] * inv;
      p[tid * ATT_PLD + j] = pv;
      P[((int64_t)b * NT + tid) * NT + j] = pv;
    }
  }
  __syncthreads();
  for (int o = tid; o < NT * TD; o += 256) {
    const int i = o >> 6, d = o & 63;
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j) a = fmaf(rbf(p[i * ATT_PLD + j], bf), v[j * ATT_LD + d], a);
    ctx[(int64_t)b * NT * TD + o] = a;
  }
}

// Backward of the above: given dctx, saved P and qkv -> dqkv (same packed layout).
//   dV = P^T dctx ; dP = dctx V^T ; dS = P o (dP - rowsum(P o dP)) ; dQ = dS K / 8 ; dK = dS^T Q / 8
template <int NT>
__global__ __launch_bounds__(256) void attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ P,
                                                       const float* __restrict__ dctx, int n,
                                                       float* __restrict__ dqkv, int bf) {
  __shared__ float q[NT * ATT_LD], k[NT * ATT_LD], v[NT * ATT_LD], dc[NT * ATT_LD];
  __shared__ float p[NT * ATT_PLD], ds[NT * ATT_PLD];
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const float* src = qkv + (int64_t)b * NT * 3 * TD;
  for (int idx = tid; idx < NT * 3 * TD; idx += 256) {
    const int t = idx / (3 * TD), c = idx - t * 3 * TD;
    const int part = c >> 6, d = c & 63;
    (part == 0 ? q : part == 1 ? k : v)[t * ATT_LD + d] = rbf(src[idx], bf);  // q, k, v, dctx: contraction operands only
  }
  for (int o = tid; o < NT * TD; o += 256) dc[(o >> 6) * ATT_LD + (o & 63)] = rbf(dctx[(int64_t)b * NT * TD + o], bf);
  for (int pr = tid; pr < NT * NT; pr += 256) {
    const int i = pr / NT, j = pr - i * NT;
    p[i * ATT_PLD + j] = P[(int64_t)b * NT * NT + pr];
  }
  __syncthreads();
  float* dst = dqkv + (int64_t)b * NT * 3 * TD;
  for (int o = tid; o < NT * TD; o += 256) {  // dV[j][d]
    const int j = o >> 6, d = o & 63;
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < NT; ++i) a = fmaf(rbf(p[i * ATT_PLD + j], bf), dc[i * ATT_LD + d], a);
    dst[j * 3 * TD + 2 * TD + d] = a;
  }
  for (int pr = tid; pr < NT * NT; pr += 256) {  // dP[i][j]
    const int i = pr / NT, j = pr - i * NT;
    float s = 0.f;
#pragma unroll 16
    for (int d = 0; d < TD; ++d) s = fmaf(dc[i * ATT_LD + d], v[j * ATT_LD + d], s);
    ds[i * ATT_PLD + j] = s;
  }
  __syncthreads();
  if (tid < NT) {
    float rd = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j) rd = fmaf(p[tid * ATT_PLD + j], ds[tid * ATT_PLD + j], rd);
#pragma unroll
    for (int j = 0; j < NT; ++j) ds[tid * ATT_PLD + j] = p[tid * ATT_PLD + j] * (ds[tid * ATT_PLD + j] - rd);
  }
  __syncthreads();
  for (int o = tid; o < NT * TD; o += 256) {
    const int t = o >> 6, d = o & 63;
    float aq = 0.f, ak = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      aq = fmaf(rbf(ds[t * ATT_PLD + j], bf), k[j * ATT_LD + d], aq);  // dQ[t][d] = sum_j dS[t][j] K[j][d]
      ak = fmaf(rbf(ds[j * ATT_PLD + t], bf), q[j * ATT_LD + d], ak);  // dK[t][d] = sum_i dS[i][t] Q[i][d]
    }
    dst[t * 3 * TD + d] = aq * 0.125f;
    dst[t * 3 * TD + TD + d] = ak * 0.125f;
  }
}

// --------------------------------------------------------------------------------- residual + LayerNorm
// out = LN(x + y) * gamma + beta over 64 columns, eps 1e-5, biased variance (nn.LayerNorm inside
// nn.TransformerEncoderLayer, post-norm). Saves xhat and rstd for the backward. One wave per row.
__global__ __launch_bounds__(256) void add_ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int rows,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float* __restrict__ out, float* __restrict__ xhat,
                                                         float* __restrict__ rstd) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int64_t o = (int64_t)r * TD + lane;
  const float z = x[o] + y[o];
  const float mean = wave_sum(z) * (1.f / TD);
  const float c = z - mean;
  const float var = wave_sum(c * c) * (1.f / TD);
  const float rs = 1.f / sqrtf(var + 1e-5f);
  const float xh = c * rs;
  xhat[o] = xh;
  out[o] = fmaf(xh, gamma[lane], beta[lane]);
  if (lane == 0) rstd[r] = rs;
}

// d(x+y) from dout (in place allowed: dz may alias dout); per-block dgamma/dbeta partials.
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ xhat,
                                                     const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                     int rows, float* __restrict__ dz, float* __restrict__ gpart,
                                                     float* __restrict__ bpart) {
  // each block leaves its partial dgamma/dbeta in gpart/bpart[blockIdx.x][64]; wgrad_reduce_kernel sums them in a
  // fixed order (no atomics: the whole update is run-to-run deterministic). Each wave walks many rows: four rows are
  // kept in flight per iteration to overlap their load -> reduce -> store chains
  __shared__ float sg[4][TD], sb[4][TD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float g = gamma[lane];
  float ag = 0.f, ab = 0.f;
  for (int r0 = (blockIdx.x * 4 + w) * 4; r0 < rows; r0 += gridDim.x * 16) {
    float d[4], xh[4], rs[4], dxh[4], c1[4], c2[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool ok = r0 + u < rows;
      const int64_t o = (int64_t)(ok ? r0 + u : 0) * TD + lane;
      const float dd = dout[o], xx = xhat[o];
      rs[u] = rstd[ok ? r0 + u : 0];
      d[u] = ok ? dd : 0.f;
      xh[u] = ok ? xx : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      ag = fmaf(d[u], xh[u], ag);
      ab += d[u];
      dxh[u] = d[u] * g;
      c1[u] = dxh[u];
      c2[u] = dxh[u] * xh[u];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        c1[u] += __shfl_xor(c1[u], o, 64);
        c2[u] += __shfl_xor(c2[u], o, 64);
      }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (r0 + u < rows)
        dz[(int64_t)(r0 + u) * TD + lane] = rs[u] * (dxh[u] - c1[u] * (1.f / TD) - xh[u] * (c2[u] * (1.f / TD)));
  }
  sg[w][lane] = ag;
  sb[w][lane] = ab;
  __syncthreads();
  if (w == 0) {
    gpart[blockIdx.x * TD + lane] = (sg[0][lane] + sg[1][lane]) + (sg[2][lane] + sg[3][lane]);
    bpart[blockIdx.x * TD + lane] = (sb[0][lane] + sb[1][lane]) + (sb[2][lane] + sb[3][lane]);
  }
}

// --------------------------------------------------------------------------------- token pooling
// [state token | mean of the 16 depth tokens] -> [n][128]  (torchrl/networks/nets.py:1015-1021,1034); mx: the max over the
// depth tokens instead (max_pool=True, nets.py:1022-1023: `.max(dim=0)[0]`)
__global__ __launch_bounds__(128) void pool_fwd_kernel(const float* __restrict__ x, int n, float* __restrict__ pooled, int mx) {
  const int b = blockIdx.x, t = threadIdx.x;
  if (b >= n) return;
  const float* xb = x + (int64_t)b * NTOK * TD;
  float o;
  if (t < TD) o = xb[t];
  else {
    const int d = t - TD;
    float s = mx ? -INFINITY : 0.f;
#pragma unroll
    for (int i = 1; i < NTOK; ++i) s = mx ? fmaxf(s, xb[i * TD + d]) : s + xb[i * TD + d];
    o = mx ? s : s * (1.f / 16.f);
  }
  pooled[(int64_t)b * 2 * TD + t] = o;
}
// mx: the gradient of a max goes to the (first) token that attained it (torch.max(dim) backward), found again from the
// layer stack's output rows x
__global__ __launch_bounds__(64) void pool_bwd_kernel(const float* __restrict__ dpooled, int n, float* __restrict__ dx,
                                                      const float* __restrict__ x, int mx) {
  const int b = blockIdx.x, d = threadIdx.x;
  if (b >= n) return;
  const float ds = dpooled[(int64_t)b * 2 * TD + d];
  const float dg = dpooled[(int64_t)b * 2 * TD + TD + d];
  float* o = dx + (int64_t)b * NTOK * TD;
  o[d] = ds;
  if (!mx) {
    const float dm = dg * (1.f / 16.f);
#pragma unroll
    for (int i = 1; i < NTOK; ++i) o[i * TD + d] = dm;
    return;
  }
  const float* xb = x + (int64_t)b * NTOK * TD;
  int arg = 1;
  float best = xb[TD + d];
  for (int i = 2; i < NTOK; ++i) {
    const float v = xb[i * TD + d];
    if (v > best) { best = v; arg = i; }
  }
  for (int i = 1; i < NTOK; ++i) o[i * TD + d] = i == arg ? dg : 0.f;
}

// vision-only Transformer (torchrl/networks/nets.py:884-889: out[0 : 1 + 16].mean(dim=0) over a 16-token sequence is the
// mean of all tokens; max_pool=True: their max) -> [n][64]. srows: rows between two samples' first tokens (ntok when the token
// rows are dense; 17 with x pointing at row 1 of a 17-row slot: the wave-per-sample kernels' layout)
__global__ __launch_bounds__(64) void pool_all_fwd_kernel(const float* __restrict__ x, int n, int ntok, int srows,
                                                          float* __restrict__ pooled, int mx) {
  const int b = blockIdx.x, d = threadIdx.x;
  if (b >= n) return;
  const float* xb = x + (int64_t)b * srows * TD;
  float s = mx ? -INFINITY : 0.f;
  for (int i = 0; i < ntok; ++i) s = mx ? fmaxf(s, xb[i * TD + d]) : s + xb[i * TD + d];
  pooled[(int64_t)b * TD + d] = mx ? s : s * (1.f / (float)ntok);
}
__global__ __launch_bounds__(64) void pool_all_bwd_kernel(const float* __restrict__ dpooled, int n, int ntok, int srows,
                                                          float* __restrict__ dx, const float* __restrict__ x, int mx) {
  const int b = blockIdx.x, d = threadIdx.x;
  if (b >= n) return;
  const float dg = dpooled[(int64_t)b * TD + d];
  float* o = dx + (int64_t)b * srows * TD;
  if (!mx) {
    const float dm = dg * (1.f / (float)ntok);
    for (int i = 0; i < ntok; ++i) o[i * TD + d] = dm;
    return;
  }
  const float* xb = x + (int64_t)b * srows * TD;
  int arg = 0;
  float best = xb[d];
  for (int i = 1; i < ntok; ++i) {
    const float v = xb[i * TD + d];
    if (v > best) { best = v; arg = i; }
  }
  for (int i = 0; i < ntok; ++i) o[i * TD + d] = i == arg ? dg : 0.f;
}

// --------------------------------------------------------------------------------- rollout step (actor)
// Device-side cursor of the rollout: env step t of the epoch owns rollout slots [t*E, (t+1)*E).
// done: blocks of the step's last kernel that have finished. seq / stage / err: the hand-over counters of rollout_dense_kernel
// (csrc/rollout_dense.h) — monotonic, never reset; the actor's control block starts zeroed (v4l_actor_bind)
struct ActCtl { long long t; unsigned long long done; unsigned seq, err; unsigned stage[6]; };
__global__ void act_set_kernel(ActCtl* c, long long t) { c->t = t; c->done = 0; }
__global__ __launch_bounds__(256) void act_begin_kernel(const ActCtl* __restrict__ c, int E, int* __restrict__ rowidx) {
  const long long t = c->t;
  for (int i = threadIdx.x; i < E; i += 256) rowidx[i] = (int)(t * E + i);
}
// TanhNormal (policies/distribution.py:5-80): the pre-tanh value of a stored action, `log((1 + a) / (1 - a)) / 2`, and the
// per-dimension change-of-variables term `log(1 - a * a + epsilon)`, epsilon = 1e-6 — the reference's expressions
constexpr float TANH_EPS = 1e-6f;
__device__ __forceinline__ float tanh_pre(float a) { return logf((1.f + a) / (1.f - a)) / 2.f; }
__device__ __forceinline__ float tanh_corr(float a) { return logf(1.f - a * a + TANH_EPS); }

// GaussianContPolicyBase.explore (continuous_policy.py:85-125) + the value read-out of the collector
// (collector/on_policy.py:95-100) for one env step: action = mean + std * eps (== Normal(mean,std).sample() given the
// same standard-normal draws), entropy, value; also files action and value into the rollout arrays and advances t.
// SD (GaussianContPolicy, continuous_policy.py:222-236): log sigma is columns A .. 2A-1 of the row's own head output, `logstd` unused
template <bool SD>
__device__ __forceinline__ void act_finish_body(ActCtl* c, const float* __restrict__ meanp,
                                                const float* __restrict__ logstd, const float* __restrict__ valuep,
                                                const float* __restrict__ eps, int E, int A,
                                                float* __restrict__ acts_roll, float* __restrict__ values_roll,
                                                float* __restrict__ logp_roll, float* __restrict__ action,
                                                float* __restrict__ mean, float* __restrict__ stdv,
                                                float* __restrict__ ent, float* __restrict__ value, int tanh_action) {
  const long long t = c->t;
  for (int i = threadIdx.x; i < E; i += 256) {
    float e = 0.f, lp = 0.f;
    for (int a = 0; a < A; ++a) {
      const float ls = fminf(fmaxf(SD ? meanp[(int64_t)i * OUT_LD + A + a] : logstd[a], LOG_SIG_MIN), LOG_SIG_MAX);
      const float sg = expf(ls);
      e += 0.5f + HALF_LOG_2PI + logf(sg);
      const float mu = meanp[(int64_t)i * OUT_LD + a];
      float act = fmaf(sg, eps[(int64_t)i * A + a], mu);
      if (tanh_action) act = tanhf(act);  // TanhNormal.rsample (distribution.py:61-80); eps = 0: eval_act's tanh(mean)
      action[(int64_t)i * A + a] = act;
      mean[(int64_t)i * A + a] = mu;
      stdv[(int64_t)i * A + a] = sg;
      if (acts_roll != nullptr) acts_roll[(t * E + i) * A + a] = act;
      // log pi(a|s) of the acting policy, with the expression actor_loss_kernel uses for the frozen target policy:
      // the policy that acts during an epoch IS that epoch's target policy (ppo.py:34 copies it before the updates).
      // tanh policies: through the STORED action like target_pf.update(obs, actions) does (distribution.py:38-51)
      const float d = (tanh_action ? tanh_pre(act) : act) - mu;
      lp += -(d * d) / (2.f * sg * sg) - logf(sg) - HALF_LOG_2PI;
      if (tanh_action) lp -= tanh_corr(act);
    }
    ent[i] = e;
    const float v = valuep[(int64_t)i * OUT_LD];
    value[i] = v;
    if (values_roll != nullptr) values_roll[t * E + i] = v;
    if (logp_roll != nullptr) logp_roll[t * E + i] = lp;
  }
  __syncthreads();
  if (threadIdx.x == 0) c->t = t + 1;
}
__global__ __launch_bounds__(256) void act_finish_kernel(ActCtl* c, const float* __restrict__ meanp,
                                                         const float* __restrict__ logstd, const float* __restrict__ valuep,
                                                         const float* __restrict__ eps, int E, int A,
                                                         float* __restrict__ acts_roll, float* __restrict__ values_roll,
                                                         float* __restrict__ logp_roll, float* __restrict__ action,
                                                         float* __restrict__ mean, float* __restrict__ stdv,
                                                         float* __restrict__ ent, float* __restrict__ value, int tanh_action) {
  act_finish_body<false>(c, meanp, logstd, valuep, eps, E, A, acts_roll, values_roll, logp_roll, action, mean, stdv, ent, value,
                         tanh_action);
}
// the same for a policy whose head row carries its own log sigma (v4l_net_cfg.has_logstd == V4L_LOGSTD_HEAD): sigma, entropy
// and log-prob per row
__global__ __launch_bounds__(256) void act_finish_sd_kernel(ActCtl* c, const float* __restrict__ outp,
                                                            const float* __restrict__ valuep, const float* __restrict__ eps, int E,
                                                            int A, float* __restrict__ acts_roll, float* __restrict__ values_roll,
                                                            float* __restrict__ logp_roll, float* __restrict__ action,
                                                            float* __restrict__ mean, float* __restrict__ stdv,
                                                            float* __restrict__ ent, float* __restrict__ value, int tanh_action) {
  act_finish_body<true>(c, outp, nullptr, valuep, eps, E, A, acts_roll, values_roll, logp_roll, action, mean, stdv, ent, value,
                        tanh_action);
}

// --------------------------------------------------------------------------------- categorical head (discrete actions)
// CategoricalDisPolicy (policies/discrete_policies.py:127-172): the K = out_dim columns of a padded head row [OUT_LD] are logits;
// `torch.softmax(logits, -1)` feeds torch.distributions.Categorical. One thread holds a row's K values in registers: the
// log-softmax by max-subtraction, p_j = exp(z_j - max) / sum, log p_j = z_j - max - log(sum), H = -sum_j p_j log p_j, fp32
// throughout. Columns K .. 15 come out as p = 0, log p = 0. (Categorical(probs=...) clamps the probabilities to
// [eps, 1 - eps] before it takes their log: not reproduced, inactive while every p_j lies inside that interval.)
constexpr int CAT_CAP = OUT_LD;  // 2 <= K <= V4L_OUT_LD (v4l_net_set_categorical)
struct CatDist { float p[CAT_CAP], lg[CAT_CAP]; float ent; };
__device__ __forceinline__ CatDist cat_dist(const float* __restrict__ row, int K) {
  CatDist d;
  float z[CAT_CAP];
#pragma unroll
  for (int q = 0; q < CAT_CAP / 4; ++q) {  // (the rows are 64-byte aligned)
    const float4 m = *reinterpret_cast<const float4*>(row + 4 * q);
    z[4 * q] = m.x; z[4 * q + 1] = m.y; z[4 * q + 2] = m.z; z[4 * q + 3] = m.w;
  }
  float mx = z[0];
#pragma unroll
  for (int j = 1; j < CAT_CAP; ++j)
    if (j < K) mx = fmaxf(mx, z[j]);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < CAT_CAP; ++j) {
    d.p[j] = j < K ? expf(z[j] - mx) : 0.f;
    s += d.p[j];
  }
  const float ls = logf(s);
  d.ent = 0.f;
#pragma unroll
  for (int j = 0; j < CAT_CAP; ++j) {
    d.lg[j] = j < K ? z[j] - mx - ls : 0.f;
    d.p[j] = d.p[j] / s;
    d.ent -= d.p[j] * d.lg[j];
  }
  return d;
}
// log p of the action index a stored as a float; NaN for anything that is not an integer in [0, K) (register select: no indexing)
__device__ __forceinline__ float cat_logp(const CatDist& d, int K, float a) {
  float lp = NAN;
#pragma unroll
  for (int j = 0; j < CAT_CAP; ++j)
    if (j < K && a == (float)j) lp = d.lg[j];
  return lp;
}
// Categorical.sample() by inverse CDF from one uniform u in [0, 1): the first k whose running sum p_0 + .. + p_k exceeds u.
// The fp32 sum of a row can end at or below the largest uniform, 1 - 2^-24 (torch.rand draws multiples of 2^-24), and then no k
// does: the pick is the last k with p_k > 0 — never a class of probability zero, which torch.multinomial cannot return either —
// and K - 1 only for a row without one. u < 0: no draw, the first argmax (eval_act, discrete_policies.py:156-158).
__device__ __forceinline__ int cat_pick(const CatDist& d, int K, float u) {
  int idx = K - 1;
  if (u < 0.f) {
    float best = d.p[0];
    idx = 0;
#pragma unroll
    for (int j = 1; j < CAT_CAP; ++j)
      if (j < K && d.p[j] > best) { best = d.p[j]; idx = j; }
    return idx;
  }
  float c = 0.f;
  int last = K - 1;  // the last k with p_k > 0 (register select: no indexing)
  bool found = false;
#pragma unroll
  for (int j = 0; j < CAT_CAP; ++j) {
    c += d.p[j];
    if (j < K && d.p[j] > 0.f) last = j;
    if (!found && j < K && c > u) { idx = j; found = true; }
  }
  return found ? idx : last;
}
// the same pick from a row of probabilities [K] (v4l_cat_sample: what explore() draws from)
__global__ __launch_bounds__(256) void cat_sample_kernel(const float* __restrict__ probs, const float* __restrict__ u, int n, int K,
                                                         int deterministic, long long* __restrict__ idx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  CatDist d;
#pragma unroll
  for (int j = 0; j < CAT_CAP; ++j) d.p[j] = j < K ? probs[(int64_t)i * K + j] : 0.f;
  idx[i] = cat_pick(d, K, deterministic ? -1.f : u[i]);
}
// CategoricalDisPolicy.explore (discrete_policies.py:140-154) + the value read-out of the collector for one env step on the
// GENERAL route: act_finish_kernel's counterpart. u: [E] uniforms in [0, 1) (negative: argmax). Files the action index (as a
// float, [E][1] rows), the value and log pi_old, advances t; no mean / std.
__global__ __launch_bounds__(256) void act_finish_cat_kernel(ActCtl* c, const float* __restrict__ logits,
                                                             const float* __restrict__ valuep, const float* __restrict__ u, int E,
                                                             int K, float* __restrict__ acts_roll, float* __restrict__ values_roll,
                                                             float* __restrict__ logp_roll, float* __restrict__ action,
                                                             float* __restrict__ ent, float* __restrict__ value) {
  const long long t = c->t;
  for (int i = threadIdx.x; i < E; i += 256) {
    const CatDist d = cat_dist(logits + (int64_t)i * OUT_LD, K);
    const float act = (float)cat_pick(d, K, u[i]);
    action[i] = act;
    ent[i] = d.ent;
    if (acts_roll != nullptr) acts_roll[t * E + i] = act;
    const float v = valuep[(int64_t)i * OUT_LD];
    value[i] = v;
    if (values_roll != nullptr) values_roll[t * E + i] = v;
    if (logp_roll != nullptr) logp_roll[t * E + i] = cat_logp(d, K, act);
  }
  __syncthreads();
  if (threadIdx.x == 0) c->t = t + 1;
}

// --------------------------------------------------------------------------------- block reductions
struct Red4 { double s, s2; float mx, mn; };
// Block reduction (blockDim.x = 64 * nw, nw <= 16) of (sum, sum of squares, max, min); result valid on all threads.
__device__ __forceinline__ Red4 block_red4(double s, double s2, float mx, float mn) {
  __shared__ double rs[16], rs2[16];
  __shared__ float rmx[16], rmn[16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    s2 += __shfl_xor(s2, o, 64);
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    mn = fminf(mn, __shfl_xor(mn, o, 64));
  }
  __syncthreads();  // protect reuse across consecutive calls
  if (lane == 0) { rs[w] = s; rs2[w] = s2; rmx[w] = mx; rmn[w] = mn; }
  __syncthreads();
  Red4 r;
  r.s = 0.0; r.s2 = 0.0; r.mx = -INFINITY; r.mn = INFINITY;
  const int nw = blockDim.x >> 6;
  for (int k = 0; k < nw; ++k) {  // fixed order: deterministic
    r.s += rs[k]; r.s2 += rs2[k];
    r.mx = fmaxf(r.mx, rmx[k]); r.mn = fminf(r.mn, rmn[k]);
  }
  return r;
}

// Layout of the 24-float statistics record one PPO minibatch update produces. [0..17] are the 18 logger
// keys of torchrl/algo/on_policy/ppo.py:77-92,122-123,142-145 in that order; the rest is internal.
enum {
  ST_ADV_MEAN = 0, ST_ADV_STD, ST_ADV_MAX, ST_ADV_MIN, ST_VF_LOSS, ST_GN_VF, ST_PI_LOSS,
  ST_LP_MEAN, ST_LP_STD, ST_LP_MAX, ST_LP_MIN, ST_LS_MEAN, ST_LS_STD, ST_LS_MAX, ST_LS_MIN,
  ST_RATIO_MAX, ST_RATIO_MIN, ST_GN_PF,
  // per-shard moments for the data-parallel exchange: sum a, M2 = sum (a - mean_shard)^2, count, count * mean_shard^2
  // (the global variance is rebuilt as (sum M2_i + sum n_i mean_i^2 - N mean^2) / (N - 1): the only cancellation left is
  // between shard means, not between a raw sum of squares and N mean^2)
  ST_ADV_SUM = 18, ST_ADV_M2, ST_ADV_CNT, ST_ADV_NM2,
  ST_NONFINITE = 22,  // how many of the 18 logged scalars of this update are NaN / Inf (the on-device form of the
                      // collector's "NaN detected" check, collector/on_policy.py:102-107: the host reads one number per epoch)
  ST_F16_SAT = 23,    // V4L_F16: how many loss-gradient elements of this update were clamped at +-V4L_F16_GRAD_CLAMP
  ST_SIZE = 24
};

// advs.mean(), advs.std() (Bessel), max, min of the minibatch (ppo.py:142-145). Single block.
__device__ __forceinline__ void adv_stats_body(const float* __restrict__ adv, const int* rowidx, int n, float* __restrict__ st) {
  double s = 0.0; float mx = -INFINITY, mn = INFINITY;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float a = adv[rowidx ? rowidx[i] : i];
    s += a; mx = fmaxf(mx, a); mn = fminf(mn, a);
  }
  Red4 r = block_red4(s, 0.0, mx, mn);
  const double mean = r.s / n;
  double q = 0.0, sq = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const double a = adv[rowidx ? rowidx[i] : i];
    q += (a - mean) * (a - mean);
    sq += a * a;
  }
  Red4 r2 = block_red4(q, sq, 0.f, 0.f);
  if (threadIdx.x == 0) {
    st[ST_ADV_MEAN] = (float)mean;
    st[ST_ADV_STD] = (float)sqrt(r2.s / (double)(n - 1));
    st[ST_ADV_MAX] = r.mx;
    st[ST_ADV_MIN] = r.mn;
    st[ST_ADV_SUM] = (float)r.s;
    st[ST_ADV_M2] = (float)r2.s;
    st[ST_ADV_CNT] = (float)n;
    st[ST_ADV_NM2] = (float)(n * mean * mean);
  }
}
// the same statistics from values a block already holds in registers (thread t: elements t, t + blockDim, ... — the order
// adv_stats_body's loops add them in, so the bits are the same)
__device__ __forceinline__ void adv_stats_regs(const float (&a)[4], const bool (&ok)[4], int n, float* __restrict__ st) {
  double s = 0.0; float mx = -INFINITY, mn = INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (ok[j]) { s += a[j]; mx = fmaxf(mx, a[j]); mn = fminf(mn, a[j]); }
  Red4 r = block_red4(s, 0.0, mx, mn);
  const double mean = r.s / n;
  double q = 0.0, sq = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (ok[j]) { const double d = a[j]; q += (d - mean) * (d - mean); sq += d * d; }
  Red4 r2 = block_red4(q, sq, 0.f, 0.f);
  if (threadIdx.x == 0) {
    st[ST_ADV_MEAN] = (float)mean;
    st[ST_ADV_STD] = (float)sqrt(r2.s / (double)(n - 1));
    st[ST_ADV_MAX] = r.mx;
    st[ST_ADV_MIN] = r.mn;
    st[ST_ADV_SUM] = (float)r.s;
    st[ST_ADV_M2] = (float)r2.s;
    st[ST_ADV_CNT] = (float)n;
    st[ST_ADV_NM2] = (float)(n * mean * mean);
  }
}
__global__ __launch_bounds__(256) void adv_stats_kernel(const float* __restrict__ adv, const int* __restrict__ rowidx, int n,
                                                        float* __restrict__ st) {
  adv_stats_body(adv, rowidx, n, st);
}
// Data-parallel: mean / unbiased std of the GLOBAL minibatch from the all-reduced shard moments.
__global__ void adv_stats_finalize_kernel(float* st) {
  const double s = st[ST_ADV_SUM], m2 = st[ST_ADV_M2], c = st[ST_ADV_CNT], nm2 = st[ST_ADV_NM2];
  const double mean = s / c;
  st[ST_ADV_MEAN] = (float)mean;
  st[ST_ADV_STD] = (float)sqrt(fmax(0.0, (m2 + (nm2 - c * mean * mean)) / (c - 1.0)));
}
// The scalars that ride in the tail of a gradient bucket through its all-reduce (8 floats behind the gradients):
//   critic bucket: [sum a, M2, count, count * mean^2, vf_loss share, 0, 0, 0]   policy bucket: [policy_loss share, 0 ...]
// pack = 1: record -> tail (before the collective); pack = 0: tail -> record (after it). A share is the shard's value / world:
// the sum over ranks is the big-batch mean the reference would log.
// V4L_BUCKET_TAIL (= 8) comes from include/v4l_hip.h
__global__ void bucket_tail_kernel(float* __restrict__ st, float* __restrict__ tail, int which, int pack, float inv_world) {
  const int t = threadIdx.x;
  if (t >= V4L_BUCKET_TAIL) return;
  if (which == 1) {  // critic
    const int src[5] = {ST_ADV_SUM, ST_ADV_M2, ST_ADV_CNT, ST_ADV_NM2, ST_VF_LOSS};
    if (pack) tail[t] = t < 5 ? st[src[t]] : 0.f;   // vf_loss is already a share: critic_loss_kernel scales by 1 / (n * world)
    else if (t < 5) st[src[t]] = tail[t];
  } else {
    if (pack) tail[t] = t == 0 ? st[ST_PI_LOSS] * inv_world : 0.f;
    else if (t == 0) st[ST_PI_LOSS] = tail[0];
  }
}

// Communicator self-test (v4l_trainer_comm_selftest): a rank-dependent pattern of small integers — exact in fp32 whatever
// order a collective adds them in — into a gradient bucket and the record fields its tail carries, and the check of the
// all-reduced result against the sum every rank can compute on its own.
__device__ __forceinline__ float comm_pattern(int64_t i, int rank) { return (float)((i * 7 + (int64_t)rank * 13) % 251); }
__global__ __launch_bounds__(256) void comm_pattern_kernel(float* __restrict__ g, int64_t n, int rank, float* __restrict__ st,
                                                           int which) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) g[i] = comm_pattern(i, rank);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (which == 1) {
      st[ST_ADV_SUM] = (float)(rank + 1); st[ST_ADV_M2] = (float)(2 * rank + 1); st[ST_ADV_CNT] = 64.f;
      st[ST_ADV_NM2] = (float)(rank + 3); st[ST_VF_LOSS] = (float)(rank + 5);
    } else {
      st[ST_PI_LOSS] = (float)(rank + 1);
    }
  }
}
__global__ __launch_bounds__(256) void comm_check_kernel(const float* __restrict__ g, int64_t n, int world,
                                                         const float* __restrict__ st, int which, int* __restrict__ bad) {
  int mine = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float want = 0.f;
    for (int r = 0; r < world; ++r) want += comm_pattern(i, r);
    mine += g[i] != want;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const float w = (float)world, tri = 0.5f * w * (w - 1.f);  // sum of the ranks
    if (which == 1) {
      mine += st[ST_ADV_SUM] != tri + w;
      mine += st[ST_ADV_M2] != 2.f * tri + w;
      mine += st[ST_ADV_CNT] != 64.f * w;
      mine += st[ST_ADV_NM2] != tri + 3.f * w;
      mine += st[ST_VF_LOSS] != tri + 5.f * w;
    } else {
      mine += fabsf(st[ST_PI_LOSS] - (tri + w) / w) > 1e-5f * (tri + w) / w;  // shares: mean over the ranks
    }
  }
  if (mine) atomicAdd(bad, mine);
}

// (per-statement contraction for the loss rows: the statistics block and the blocks that run the heads' chain beside it
// evaluate the same row in different kernels / instantiations and must produce the same bits — see csrc/wps.h)
#pragma clang fp contract(on)
// nn.MSELoss()(values, est_rets) and its gradient (ppo.py:94-123; clipped_value_loss=False path, and the
// clipped variant of ppo.py:105-112 when clip > 0). values is the critic output [n][OUT_LD], column 0.
// One row: loss term l and d(loss)/d(value) g. (Shared by the statistics block and by the blocks that run the heads'
// data-grads beside it, csrc/wps.h: both must see the same bits.)
// A loss-gradient element as the backward's contractions get it: x gscale (1, or V4L_F16's power of two: exact) and, scaled, kept
// inside half's range (a NaN stays a NaN). sat counts the clamped ones.
__device__ __forceinline__ float grad_out(float g, float gscale, int& sat) {
  if (gscale == 1.f) return g;
  const float x = g * gscale;
  const bool over = fabsf(x) > V4L_F16_GRAD_CLAMP;
  sat += over ? 1 : 0;
  return over ? copysignf(V4L_F16_GRAD_CLAMP, x) : x;
}
__device__ __forceinline__ void critic_row(float v, float r, float ov, int clipped, float clip, float inv_n, float& l, float& g) {
  if (!clipped) {
    const float d = v - r;
    l = d * d;
    g = 2.f * d * inv_n;
  } else {
    const float dv = v - ov;
    const float vc = ov + fminf(fmaxf(dv, -clip), clip);
    const float l1 = (v - r) * (v - r), l2 = (vc - r) * (vc - r);
    // 0.5 * max(l1, l2).mean(); torch.max splits ties evenly between both arguments
    const float g1 = 2.f * (v - r);
    const float g2 = (dv >= -clip && dv <= clip) ? 2.f * (vc - r) : 0.f;
    l = 0.5f * fmaxf(l1, l2);
    g = 0.5f * inv_n * (l1 > l2 ? g1 : (l1 < l2 ? g2 : 0.5f * (g1 + g2)));
  }
}
__device__ __forceinline__ void critic_loss_body(const float* __restrict__ values, const float* __restrict__ ret,
                                                 const float* __restrict__ oldv, const int* __restrict__ rowidx, int n,
                                                 float inv_n, int clipped, float clip, float* __restrict__ dvalues,
                                                 float* __restrict__ st, float gscale) {
  double s = 0.0;
  int sat = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int slot = rowidx ? rowidx[i] : i;
    const float v = values[(int64_t)i * OUT_LD], r = ret[slot];
    float g, l;
    critic_row(v, r, clipped ? oldv[slot] : 0.f, clipped, clip, inv_n, l, g);
    g = grad_out(g, gscale, sat);
    s += l;
#pragma unroll
    for (int c = 0; c < OUT_LD; ++c) dvalues[(int64_t)i * OUT_LD + c] = c == 0 ? g : 0.f;
  }
  Red4 r = block_red4(s, (double)sat, 0.f, 0.f);
  if (threadIdx.x == 0) {
    st[ST_VF_LOSS] = (float)(r.s * (double)inv_n);
    if (gscale != 1.f) st[ST_F16_SAT] += (float)r.s2;
  }
}
__global__ __launch_bounds__(1024) void critic_loss_kernel(const float* __restrict__ values, const float* __restrict__ ret,
                                                          const float* __restrict__ oldv, const int* __restrict__ rowidx,
                                                          int n, float inv_n, int clipped, float clip,
                                                          float* __restrict__ dvalues, float* __restrict__ st, float gscale) {
  critic_loss_body(values, ret, oldv, rowidx, n, inv_n, clipped, clip, dvalues, st, gscale);
}


// Clipped-surrogate + entropy loss of PPO.update_actor (ppo.py:42-92) and its gradient w.r.t. the policy
// mean [n][OUT_LD] and logstd [A]. logp_old comes from the frozen target policy's mean/logstd on the same
// minibatch. Advantages are normalised with the minibatch statistics in st (ppo.py:148). Single block.
// inv_n is 1/(global batch) so that data-parallel ranks sum to the big-batch gradient.
struct ActorArgs {
  const float *mean, *logstd, *tmean, *tlogstd, *logp_old, *acts, *adv;
  const int* rowidx;
  int n, A;
  float inv_n, clip, ent_coef;
  float *dmean, *dlogstd, *st;
  float gscale;     // the dmean rows leave multiplied by this (v4l_net_grad_scale: 1, or V4L_F16's power of two); d log sigma never does
  int tanh_action;  // TanhNormal policies: log-probs of the stored (post-tanh) actions through atanh, distribution.py:38-51
};
// ACT_CAP: the compile-time action capacity of the per-row code below: 8 (every shipped config: the MPC action space, A = 6)
// or V4L_MAX_ACT = 16 (joint-space control, one action per motor: A = 12). The per-dimension arrays are per-thread state: at
// capacity 8 they fit the 128 VGPRs a 1024-thread block leaves a thread (121 used, no spill); at capacity 16 they do not (the
// compiler spills 88 VGPRs to 228 B of scratch per lane under that bound — DESIGN.md 4.5), so a policy with A <= 8 runs the
// capacity-8 instantiation and pays nothing for the wider one.
constexpr int ACT_CAP_NARROW = 8;
static_assert(V4L_MAX_ACT == OUT_LD, "the widest policy fills the padded head row exactly");
constexpr int act_cap(int A) { return A <= ACT_CAP_NARROW ? ACT_CAP_NARROW : V4L_MAX_ACT; }
template <int CAP> struct ActorDimsT { float ls[CAP], sg[CAP], lsg[CAP], tls[CAP], tsg[CAP], tlsg[CAP]; float ent; };
typedef ActorDimsT<ACT_CAP_NARROW> ActorDims;
template <int CAP = ACT_CAP_NARROW>
__device__ __forceinline__ ActorDimsT<CAP> actor_dims(const ActorArgs& p) {
  ActorDimsT<CAP> d;
  d.ent = 0.f;
#pragma unroll
  for (int a = 0; a < CAP; ++a) {
    d.ls[a] = d.sg[a] = d.lsg[a] = d.tls[a] = d.tsg[a] = d.tlsg[a] = 0.f;
    if (a < p.A) {
      d.ls[a] = fminf(fmaxf(p.logstd[a], LOG_SIG_MIN), LOG_SIG_MAX);
      d.sg[a] = expf(d.ls[a]); d.lsg[a] = logf(d.sg[a]);
      d.tls[a] = p.tlogstd != nullptr ? fminf(fmaxf(p.tlogstd[a], LOG_SIG_MIN), LOG_SIG_MAX) : 0.f;
      d.tsg[a] = expf(d.tls[a]); d.tlsg[a] = logf(d.tsg[a]);
      d.ent += 0.5f + HALF_LOG_2PI + d.lsg[a];
    }
  }
  return d;
}
// one minibatch row i (rollout slot `slot`): log pi, ratio, surrogate term, d(loss)/d(log pi) and the per-dimension factors of
// d(log pi)/d(mean) (dm) and d(log pi)/d(log sigma) + 1 (z2)
// TANH: compiled in only for TanhNormal policies (as a run-time flag the atanh / correction logs were evaluated speculatively for
// every policy: the single-block statistics launch went from 14 to 36 us)
template <int CAP> struct ActorRowT { float lp, ratio, sur, dlp, dm[CAP], z2[CAP]; };
typedef ActorRowT<ACT_CAP_NARROW> ActorRow;
// a padded [OUT_LD] row's first CAP floats: the rows are 64-byte aligned, 16-byte loads instead of A strided scalar ones
template <int CAP>
__device__ __forceinline__ void actor_load_row(const float* __restrict__ row, float (&v)[CAP]) {
#pragma unroll
  for (int q = 0; q < CAP / 4; ++q) {
    const float4 m = *reinterpret_cast<const float4*>(row + 4 * q);
    v[4 * q] = m.x; v[4 * q + 1] = m.y; v[4 * q + 2] = m.z; v[4 * q + 3] = m.w;
  }
}
template <bool TANH, int CAP = ACT_CAP_NARROW>
__device__ __forceinline__ ActorRowT<CAP> actor_row(const ActorArgs& p, const ActorDimsT<CAP>& D, int i, int slot, float amean,
                                                    float astd) {
  ActorRowT<CAP> o;
  float lp = 0.f, lpo = 0.f, mu[CAP], tmu[CAP];
  actor_load_row(p.mean + (int64_t)i * OUT_LD, mu);
  if (p.logp_old == nullptr) actor_load_row(p.tmean + (int64_t)i * OUT_LD, tmu);
#pragma unroll
  for (int a = 0; a < CAP; ++a) {
    if (a < p.A) {
      const float act = p.acts[(int64_t)slot * p.A + a];
      const float x = TANH ? tanh_pre(act) : act;
      const float corr = TANH ? tanh_corr(act) : 0.f;
      const float d = x - mu[a];
      const float var = D.sg[a] * D.sg[a];
      lp += -(d * d) / (2.f * var) - D.lsg[a] - HALF_LOG_2PI - corr;
      o.z2[a] = d * d / var;
      o.dm[a] = d / var;
      if (p.logp_old == nullptr) {
        const float dt = x - tmu[a];
        lpo += -(dt * dt) / (2.f * D.tsg[a] * D.tsg[a]) - D.tlsg[a] - HALF_LOG_2PI - corr;
      }
    } else {
      o.z2[a] = 0.f; o.dm[a] = 0.f;
    }
  }
  if (p.logp_old != nullptr) lpo = p.logp_old[slot];  // stored when the action was taken (== the target policy's)
  const float ratio = expf(lp - lpo);
  const float an = (p.adv[slot] - amean) / (astd + 1e-5f);
  const float pre = ratio * an;
  const float clp = fminf(fmaxf(ratio, 1.f - p.clip), 1.f + p.clip) * an;
  o.lp = lp; o.ratio = ratio;
  o.sur = fminf(pre, clp);
  // d(-mean(min(pre,clp)))/dlogp: the clipped branch has zero slope outside the clip range. Written
  // !(pre > clp), not pre <= clp: the same for every non-NaN pair, and a NaN advantage / ratio gives a NaN slope as torch.min's
  // backward does, instead of a silent zero that would hide it from the gradient norm (the non-finite-step guard)
  o.dlp = !(pre > clp) ? -p.inv_n * an * ratio : 0.f;
  return o;
}
// the row's d(loss)/d(mean) as the backward gets it (statistics block and chain blocks: the same bits)
template <int CAP>
__device__ __forceinline__ void actor_dmean_row(const ActorRowT<CAP>& o, float gscale, float (&dmr)[CAP], int& sat) {
#pragma unroll
  for (int a = 0; a < CAP; ++a) dmr[a] = grad_out(o.dlp * o.dm[a], gscale, sat);
}
// files a row's d(loss)/d(mean) in a padded row of >= OUT_LD floats; zero_rest: the columns from CAP on as zeros too
template <int CAP>
__device__ __forceinline__ void actor_store_dmean(float* __restrict__ row, const float (&dmr)[CAP], bool zero_rest) {
  float4* drow = reinterpret_cast<float4*>(row);
#pragma unroll
  for (int q = 0; q < CAP / 4; ++q) drow[q] = float4{dmr[4 * q], dmr[4 * q + 1], dmr[4 * q + 2], dmr[4 * q + 3]};  // dm[a >= A] == 0
  if (zero_rest) {
#pragma unroll
    for (int q = CAP / 4; q < OUT_LD / 4; ++q) drow[q] = float4{0.f, 0.f, 0.f, 0.f};
  }
}
template <bool TANH, int CAP = ACT_CAP_NARROW>
__device__ __forceinline__ void actor_loss_body(const ActorArgs& p) {
  __shared__ float sdl[16][CAP];
  const int n = p.n, A = p.A;
  const ActorDimsT<CAP> D = actor_dims<CAP>(p);
  float dl[CAP];
#pragma unroll
  for (int a = 0; a < CAP; ++a) dl[a] = 0.f;
  const float amean = p.st[ST_ADV_MEAN], astd = p.st[ST_ADV_STD];
  double s_lp = 0.0, s_lp2 = 0.0, s_sur = 0.0;
  int sat = 0;
  float lp_mx = -INFINITY, lp_mn = INFINITY, r_mx = -INFINITY, r_mn = INFINITY;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int slot = p.rowidx ? p.rowidx[i] : i;
    const ActorRowT<CAP> o = actor_row<TANH, CAP>(p, D, i, slot, amean, astd);
    s_sur += o.sur;
    {
      float dmr[CAP];
      actor_dmean_row(o, p.gscale, dmr, sat);
      actor_store_dmean(p.dmean + (int64_t)i * OUT_LD, dmr, true);
    }
#pragma unroll
    for (int a = 0; a < CAP; ++a)
      if (a < A) dl[a] += o.dlp * (o.z2[a] - 1.f);
    s_lp += o.lp; s_lp2 += (double)o.lp * o.lp;
    lp_mx = fmaxf(lp_mx, o.lp); lp_mn = fminf(lp_mn, o.lp);
    r_mx = fmaxf(r_mx, o.ratio); r_mn = fminf(r_mn, o.ratio);
  }
  Red4 r1 = block_red4(s_lp, s_lp2, lp_mx, lp_mn);
  Red4 r2 = block_red4(s_sur, (double)sat, r_mx, r_mn);
  // reduce dlogstd over the block
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < CAP; ++a) {
    float v = wave_sum(dl[a]);
    if (lane == 0) sdl[w][a] = v;
  }
  __syncthreads();
  float* st = p.st;
  if (threadIdx.x < A) {
    const int a = threadIdx.x;
    const float raw = p.logstd[a];
    float g = 0.f;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) g += sdl[k][a];
    // entropy term: -ent_coef * mean_b(sum_a log sigma_a + const); each local sample carries weight inv_n
    g += -p.ent_coef * p.inv_n * (float)n;
    p.dlogstd[a] = (raw >= LOG_SIG_MIN && raw <= LOG_SIG_MAX) ? g : 0.f;
  }
  if (threadIdx.x == 0) {
    const double lpm = r1.s / n;
    st[ST_PI_LOSS] = (float)(-(r2.s / n) - (double)p.ent_coef * D.ent);
    st[ST_LP_MEAN] = (float)lpm;
    st[ST_LP_STD] = (float)sqrt(fmax(0.0, (r1.s2 - n * lpm * lpm) / (double)(n - 1)));
    st[ST_LP_MAX] = r1.mx; st[ST_LP_MIN] = r1.mn;
    st[ST_RATIO_MAX] = r2.mx; st[ST_RATIO_MIN] = r2.mn;
    if (p.gscale != 1.f) st[ST_F16_SAT] += (float)r2.s2;
    double m = 0.0; float mx = -INFINITY, mn = INFINITY;
#pragma unroll
    for (int a = 0; a < CAP; ++a)
      if (a < A) { m += D.ls[a]; mx = fmaxf(mx, D.ls[a]); mn = fminf(mn, D.ls[a]); }
    m /= A;
    double q = 0.0;
#pragma unroll
    for (int a = 0; a < CAP; ++a)
      if (a < A) q += (D.ls[a] - m) * (D.ls[a] - m);
    st[ST_LS_MEAN] = (float)m;
    st[ST_LS_STD] = A > 1 ? (float)sqrt(q / (A - 1)) : NAN;
    st[ST_LS_MAX] = mx; st[ST_LS_MIN] = mn;
  }
}
template <bool TANH, int CAP>
__global__ __launch_bounds__(1024) void actor_loss_kernel(ActorArgs p) { actor_loss_body<TANH, CAP>(p); }

// The sibling for GaussianContPolicy (continuous_policy.py:222-236; v4l_net_cfg.has_logstd == V4L_LOGSTD_HEAD): log sigma is
// state dependent — columns A .. 2A-1 of the row's own [OUT_LD] head output (p.mean; the frozen target's in p.tmean), clamped and exponentiated per
// row — so nothing is hoisted out of the row loop, the gradient w.r.t. the raw log sigma leaves in columns A .. 2A-1 of the d(out)
// row (through grad_out like d(mean): those columns pass the backward's contractions) and log_std/* are the statistics of the
// clamped [n][A] tensor (ppo.py:84-87). p.logstd, p.tlogstd and p.dlogstd are unused. A <= ACT_CAP_NARROW. Single block.
// The mean half comes in with 16-byte loads; the log-sigma half starts at column A, unaligned for odd A and at a run-time offset:
// read as A scalar loads of the cache line the row loads just fetched, never as a run-time index into a register array.
template <bool TANH>
__device__ __forceinline__ void actor_loss_sd_body(const ActorArgs& p) {
  constexpr int CAP = ACT_CAP_NARROW;
  const int n = p.n, A = p.A;
  const bool stored = p.logp_old != nullptr;
  const float amean = p.st[ST_ADV_MEAN], astd = p.st[ST_ADV_STD];
  const float dent = p.ent_coef * p.inv_n;  // d(-ent_coef * mean_i(ent_i))/d(log sigma_ia), sign below
  double s_lp = 0.0, s_lp2 = 0.0, s_sur = 0.0, s_ent = 0.0, s_ls = 0.0, s_ls2 = 0.0;
  int sat = 0;
  float lp_mx = -INFINITY, lp_mn = INFINITY, r_mx = -INFINITY, r_mn = INFINITY, ls_mx = -INFINITY, ls_mn = INFINITY;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int slot = p.rowidx ? p.rowidx[i] : i;
    const float* __restrict__ row = p.mean + (int64_t)i * OUT_LD;
    const float* __restrict__ trow = stored ? row : p.tmean + (int64_t)i * OUT_LD;
    float mu[CAP], tmu[CAP], dm[CAP], dl[CAP];
    actor_load_row(row, mu);
    if (!stored) actor_load_row(trow, tmu);
    float lp = 0.f, lpo = 0.f, ent = 0.f;
    unsigned open = 0;  // bit a: raw log sigma_a inside [LOG_SIG_MIN, LOG_SIG_MAX] — the clamp passes its gradient
    // pass 1 over the dimensions: log pi, log pi_old, entropy, log_std statistics; keeps d / var and z^2 - 1 for pass 2
#pragma unroll
    for (int a = 0; a < CAP; ++a) {
      dm[a] = 0.f; dl[a] = 0.f;
      if (a < A) {
        const float raw = row[A + a];
        const float ls = fminf(fmaxf(raw, LOG_SIG_MIN), LOG_SIG_MAX);
        const float sg = expf(ls), lsg = logf(sg);
        const float act = p.acts[(int64_t)slot * A + a];
        const float x = TANH ? tanh_pre(act) : act;
        const float corr = TANH ? tanh_corr(act) : 0.f;
        const float d = x - mu[a];
        const float var = sg * sg;
        lp += -(d * d) / (2.f * var) - lsg - HALF_LOG_2PI - corr;
        dm[a] = d / var;
        dl[a] = d * d / var - 1.f;
        open |= (raw >= LOG_SIG_MIN && raw <= LOG_SIG_MAX) ? 1u << a : 0u;  // torch.clamp passes the gradient at both ends
        ent += 0.5f + HALF_LOG_2PI + lsg;
        s_ls += ls; s_ls2 += (double)ls * ls;
        ls_mx = fmaxf(ls_mx, ls); ls_mn = fminf(ls_mn, ls);
        if (!stored) {
          const float tls = fminf(fmaxf(trow[A + a], LOG_SIG_MIN), LOG_SIG_MAX);
          const float tsg = expf(tls), tlsg = logf(tsg);
          const float dt = x - tmu[a];
          lpo += -(dt * dt) / (2.f * tsg * tsg) - tlsg - HALF_LOG_2PI - corr;
        }
      }
    }
    if (stored) lpo = p.logp_old[slot];  // stored when the action was taken (== the target policy's)
    const float ratio = expf(lp - lpo);
    const float an = (p.adv[slot] - amean) / (astd + 1e-5f);
    const float pre = ratio * an;
    const float clp = fminf(fmaxf(ratio, 1.f - p.clip), 1.f + p.clip) * an;
    const float dlp = !(pre > clp) ? -p.inv_n * an * ratio : 0.f;  // (see actor_row)
    s_sur += fminf(pre, clp);
    s_ent += ent;
    s_lp += lp; s_lp2 += (double)lp * lp;
    lp_mx = fmaxf(lp_mx, lp); lp_mn = fminf(lp_mn, lp);
    r_mx = fmaxf(r_mx, ratio); r_mn = fminf(r_mn, ratio);
    // pass 2: the d(out) row — [d mean | d raw log sigma | zeros], every one of the OUT_LD columns written exactly once
    float* __restrict__ drow = p.dmean + (int64_t)i * OUT_LD;
#pragma unroll
    for (int a = 0; a < CAP; ++a) {
      if (a < A) {
        drow[a] = grad_out(dlp * dm[a], p.gscale, sat);
        // outside the clamp's range: exactly 0, whatever the slope (and not counted as a clamped element)
        drow[A + a] = (open >> a & 1u) ? grad_out(dlp * dl[a] - dent, p.gscale, sat) : 0.f;
      }
    }
    for (int c = 2 * A; c < OUT_LD; ++c) drow[c] = 0.f;
  }
  Red4 r1 = block_red4(s_lp, s_lp2, lp_mx, lp_mn);
  Red4 r2 = block_red4(s_sur, (double)sat, r_mx, r_mn);
  Red4 r3 = block_red4(s_ls, s_ls2, ls_mx, ls_mn);
  Red4 r4 = block_red4(s_ent, 0.0, 0.f, 0.f);
  if (threadIdx.x == 0) {
    float* st = p.st;
    const double lpm = r1.s / n;
    // -mean(sur) - ent_coef * mean_i(sum_a(0.5 + log(2 pi) / 2 + log sigma_ia))
    st[ST_PI_LOSS] = (float)(-(r2.s / n) - (double)p.ent_coef * (r4.s / n));
    st[ST_LP_MEAN] = (float)lpm;
    st[ST_LP_STD] = (float)sqrt(fmax(0.0, (r1.s2 - n * lpm * lpm) / (double)(n - 1)));
    st[ST_LP_MAX] = r1.mx; st[ST_LP_MIN] = r1.mn;
    st[ST_RATIO_MAX] = r2.mx; st[ST_RATIO_MIN] = r2.mn;
    if (p.gscale != 1.f) st[ST_F16_SAT] += (float)r2.s2;
    // log_std.mean() / .std() (Bessel, over all n * A elements) / .max() / .min() of the clamped tensor: finite at A = 1 for n >= 2
    const double cnt = (double)n * A, lsm = r3.s / cnt;
    st[ST_LS_MEAN] = (float)lsm;
    st[ST_LS_STD] = cnt > 1.0 ? (float)sqrt(fmax(0.0, (r3.s2 - cnt * lsm * lsm) / (cnt - 1.0))) : NAN;
    st[ST_LS_MAX] = r3.mx; st[ST_LS_MIN] = r3.mn;
  }
}
template <bool TANH>
__global__ __launch_bounds__(1024) void actor_loss_sd_kernel(ActorArgs p) { actor_loss_sd_body<TANH>(p); }

// The sibling for CategoricalDisPolicy (policies/discrete_policies.py:160-172: log_prob and entropy of
// Categorical(softmax(logits))) — PPODiscrete's loss launch, in actor_loss_kernel's position with its record. p.mean: the logits
// rows [n][OUT_LD] (the frozen target's in p.tmean), p.A = K, p.acts: [slots][1] action indices as floats; p.logstd, p.tlogstd,
// p.dlogstd and p.tanh_action are unused. log pi_old is the stored rollout value, or the target's log-softmax at the action.
// Per row, with p = softmax(z), H its entropy and dlp the clipped surrogate's slope of actor_row:
//   policy_loss = -mean_i(min(ratio_i an_i, clamp(ratio_i) an_i)) - ent_coef mean_i(H_i)
//   d z_j = dlp ([j == a] - p_j) + (ent_coef / n) p_j (log p_j + H)            (dH / dz_j = -p_j (log p_j + H))
// through grad_out, columns K .. 15 exactly zero. The four log_std/* slots stay as the caller cleared them. Single block.
// The target's CatDist is reduced to its one log p before the live row's is built: a thread never holds both.
__global__ __launch_bounds__(1024) void actor_loss_cat_kernel(ActorArgs p) {
  const int n = p.n, K = p.A;
  const bool stored = p.logp_old != nullptr;
  const float amean = p.st[ST_ADV_MEAN], astd = p.st[ST_ADV_STD];
  const float dent = p.ent_coef * p.inv_n;
  double s_lp = 0.0, s_lp2 = 0.0, s_sur = 0.0, s_ent = 0.0;
  int sat = 0;
  float lp_mx = -INFINITY, lp_mn = INFINITY, r_mx = -INFINITY, r_mn = INFINITY;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int slot = p.rowidx ? p.rowidx[i] : i;
    const float act = p.acts[slot];
    float lpo;
    if (stored) {
      lpo = p.logp_old[slot];  // stored when the action was taken (== the target policy's)
    } else {
      const CatDist t = cat_dist(p.tmean + (int64_t)i * OUT_LD, K);
      lpo = cat_logp(t, K, act);
    }
    const CatDist d = cat_dist(p.mean + (int64_t)i * OUT_LD, K);
    const float lp = cat_logp(d, K, act);
    const float ratio = expf(lp - lpo);
    const float an = (p.adv[slot] - amean) / (astd + 1e-5f);
    const float pre = ratio * an;
    const float clp = fminf(fmaxf(ratio, 1.f - p.clip), 1.f + p.clip) * an;
    const float dlp = !(pre > clp) ? -p.inv_n * an * ratio : 0.f;  // (see actor_row)
    s_sur += fminf(pre, clp);
    s_ent += d.ent;
    s_lp += lp; s_lp2 += (double)lp * lp;
    lp_mx = fmaxf(lp_mx, lp); lp_mn = fminf(lp_mn, lp);
    r_mx = fmaxf(r_mx, ratio); r_mn = fminf(r_mn, ratio);
    float dz[CAT_CAP];
#pragma unroll
    for (int j = 0; j < CAT_CAP; ++j) {
      dz[j] = 0.f;
      if (j < K) {
        const float hit = act == (float)j ? 1.f : 0.f;
        dz[j] = grad_out(dlp * (hit - d.p[j]) + dent * d.p[j] * (d.lg[j] + d.ent), p.gscale, sat);
      }
    }
    actor_store_dmean(p.dmean + (int64_t)i * OUT_LD, dz, true);
  }
  const Red4 r1 = block_red4(s_lp, s_lp2, lp_mx, lp_mn);
  const Red4 r2 = block_red4(s_sur, (double)sat, r_mx, r_mn);
  const Red4 r3 = block_red4(s_ent, 0.0, 0.f, 0.f);
  if (threadIdx.x == 0) {
    float* st = p.st;
    const double lpm = r1.s / n;
    st[ST_PI_LOSS] = (float)(-(r2.s / n) - (double)p.ent_coef * (r3.s / n));  // ppo.py:69 with ent.mean()
    st[ST_LP_MEAN] = (float)lpm;
    st[ST_LP_STD] = (float)sqrt(fmax(0.0, (r1.s2 - n * lpm * lpm) / (double)(n - 1)));
    st[ST_LP_MAX] = r1.mx; st[ST_LP_MIN] = r1.mn;
    st[ST_RATIO_MAX] = r2.mx; st[ST_RATIO_MIN] = r2.mn;
    if (p.gscale != 1.f) st[ST_F16_SAT] += (float)r2.s2;
  }
}

// The KL early stop of PPO(target_kl=...) (v4l_trainer_kl_stop). Runs after the actor's loss launch has completed
// the record (behind the policy's backward) and before the actor's clip_adam_kernel. Single block, row-strided.
//   approx_kl = mean_i(log pi_old(a_i|s_i)) - mean_i(log pi_theta(a_i|s_i))      ((logp_old - logp).mean(), Spinning Up's PPO)
// The second mean is the record's ST_LP_MEAN, whichever loss route wrote it. The first is the mean of the log pi_old values the
// ratio used: logp_old[slot] where the rollout stores it, otherwise the frozen target's log-probability of the stored action from
// the target's head rows (tmean; log sigma from tlogstd, or sd: from columns A .. 2A-1 of the row) — the expressions of actor_row /
// actor_loss_sd_body's lpo, spelled out again here on purpose (those kernels' row code stays where it is: DESIGN.md 7).
// Sum and subtraction in double. kl_all[u] = {approx_kl, latch after this update's decision (1.0 / 0.0)}, u = UpdCtl::upd_index (the
// closing clip_adam_kernel advances it after this launch). The latch (UpdCtl::kl_stop) is set when approx_kl > thresh
// (= 1.5 * target_kl, formed by the host in double) and never cleared here; a NaN approx_kl compares false and does not latch.
struct KlArgs {
  const float *tmean, *tlogstd, *logp_old, *acts;  // tmean / tlogstd unused with a stored logp_old; tlogstd unused with sd
  const int* rowidx;
  int n, A, sd;
  const float* st;   // the record being filled (ST_LP_MEAN)
  const int* upd_index;  // &UpdCtl::upd_index of the open run
  int* latch;            // &UpdCtl::kl_stop
  float* kl_all;         // [U][2]
  double thresh;
};
template <bool TANH>
__global__ __launch_bounds__(1024) void kl_stop_kernel(KlArgs q) {
  const int n = q.n, A = q.A;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int slot = q.rowidx ? q.rowidx[i] : i;
    float lpo = 0.f;
    if (q.logp_old != nullptr) {
      lpo = q.logp_old[slot];
    } else {
      const float* __restrict__ trow = q.tmean + (int64_t)i * OUT_LD;
      for (int a = 0; a < A; ++a) {
        const float act = q.acts[(int64_t)slot * A + a];
        const float x = TANH ? tanh_pre(act) : act;
        const float corr = TANH ? tanh_corr(act) : 0.f;
        const float tls = fminf(fmaxf(q.sd ? trow[A + a] : q.tlogstd[a], LOG_SIG_MIN), LOG_SIG_MAX);
        const float tsg = expf(tls), tlsg = logf(tsg);
        const float dt = x - trow[a];
        lpo += -(dt * dt) / (2.f * tsg * tsg) - tlsg - HALF_LOG_2PI - corr;
      }
    }
    s += (double)lpo;
  }
  const Red4 r = block_red4(s, 0.0, 0.f, 0.f);
  if (threadIdx.x == 0) {
    const double kl = r.s / (double)n - (double)q.st[ST_LP_MEAN];
    const int u = *q.upd_index;
    const int latch = (*q.latch != 0 || kl > q.thresh) ? 1 : 0;
    *q.latch = latch;
    q.kl_all[(int64_t)u * 2] = (float)kl;
    q.kl_all[(int64_t)u * 2 + 1] = latch ? 1.f : 0.f;
  }
}

// The KL-adaptive learning rates of PPO(desired_kl=...) (v4l_trainer_kl_adapt): legged_gym / rsl_rl's
// schedule = "adaptive", decided on the device. Runs where kl_stop_kernel runs in a run armed with the early stop: behind the policy's
// backward (the record is complete), in front of the actor's clip_adam_kernel. Single block, row-strided.
//   approx_kl = mean_i(log pi_old(a_i|s_i)) - mean_i(log pi_theta(a_i|s_i))      the number kl_stop_kernel forms
// with the log pi_old expressions of actor_row / actor_loss_sd_body's lpo spelled out once more, on purpose (neither the loss kernels'
// row code nor kl_stop_kernel's is shared: DESIGN.md 7). Sum and subtraction in double. The decision
//   d = -1 if approx_kl > hi (= 2 * desired_kl),  +1 if approx_kl < lo (= 0.5 * desired_kl),  0 otherwise (a NaN compares false twice)
// has no "approx_kl > 0" clause: the estimate can be negative, and a negative one raises the rates. Both rates take the decision,
// each with one double operation and its clamp:
//   d = -1: lr = fmax(lr / factor, lr_min)        d = +1: lr = fmin(lr * factor, lr_max)
// and go back into UpdCtl::lr_pf / lr_vf, which upd_begin_step reads when the NEXT update opens: this update's critic step is
// behind this launch and its policy step uses the step_size[0] / decay[0] formed when the update opened. No other launch of the
// update reads or writes the two words. rec[u] = {approx_kl, d, (float)lr_pf, (float)lr_vf} (the rates after the decision),
// u = UpdCtl::upd_index (the closing clip_adam_kernel advances it after this launch).
struct KlAdaptArgs {
  const float *tmean, *tlogstd, *logp_old, *acts;  // tmean / tlogstd unused with a stored logp_old; tlogstd unused with sd
  const int* rowidx;
  int n, A, sd;
  const float* st;       // the record being filled (ST_LP_MEAN)
  const int* upd_index;  // &UpdCtl::upd_index of the open run
  double *lr_pf, *lr_vf; // &UpdCtl::lr_pf, &UpdCtl::lr_vf
  float* rec;            // [U][4]
  double lo, hi, factor, lr_min, lr_max;
};
template <bool TANH>
__global__ __launch_bounds__(1024) void kl_adapt_kernel(KlAdaptArgs q) {
  const int n = q.n, A = q.A;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int slot = q.rowidx ? q.rowidx[i] : i;
    float lpo = 0.f;
    if (q.logp_old != nullptr) {
      lpo = q.logp_old[slot];
    } else {
      const float* __restrict__ trow = q.tmean + (int64_t)i * OUT_LD;
      for (int a = 0; a < A; ++a) {
        const float act = q.acts[(int64_t)slot * A + a];
        const float x = TANH ? tanh_pre(act) : act;
        const float corr = TANH ? tanh_corr(act) : 0.f;
        const float tls = fminf(fmaxf(q.sd ? trow[A + a] : q.tlogstd[a], LOG_SIG_MIN), LOG_SIG_MAX);
        const float tsg = expf(tls), tlsg = logf(tsg);
        const float dt = x - trow[a];
        lpo += -(dt * dt) / (2.f * tsg * tsg) - tlsg - HALF_LOG_2PI - corr;
      }
    }
    s += (double)lpo;
  }
  const Red4 r = block_red4(s, 0.0, 0.f, 0.f);
  if (threadIdx.x == 0) {
    const double kl = r.s / (double)n - (double)q.st[ST_LP_MEAN];
    const int u = *q.upd_index;
    const int d = kl > q.hi ? -1 : kl < q.lo ? 1 : 0;
    double lp = *q.lr_pf, lv = *q.lr_vf;
    if (d < 0) {
      lp = fmax(lp / q.factor, q.lr_min);
      lv = fmax(lv / q.factor, q.lr_min);
    } else if (d > 0) {
      lp = fmin(lp * q.factor, q.lr_max);
      lv = fmin(lv * q.factor, q.lr_max);
    }
    *q.lr_pf = lp;
    *q.lr_vf = lv;
    float* out = q.rec + (int64_t)u * 4;
    out[0] = (float)kl; out[1] = (float)d; out[2] = (float)lp; out[3] = (float)lv;
  }
}
#pragma clang fp contract(fast)

// Gaussian head post-processing for the policy API (continuous_policy.py:85-146,486-492): from the padded
// mean [n][OUT_LD] and logstd [A] produce contiguous mean/std [n][A], clamped log_std [A], ent [n] and, when
// acts != null, log_prob [n] of those actions.
__global__ __launch_bounds__(256) void gauss_head_kernel(const float* __restrict__ meanp, const float* __restrict__ logstd,
                                                         const float* __restrict__ acts, int n, int A,
                                                         float* __restrict__ mean, float* __restrict__ stdv,
                                                         float* __restrict__ logstd_c, float* __restrict__ ent,
                                                         float* __restrict__ logp, int tanh_action = 0,
                                                         const float* __restrict__ pre_tanh = nullptr) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  float e = 0.f, lp = 0.f;
  for (int a = 0; a < A; ++a) {
    const float ls = fminf(fmaxf(logstd[a], LOG_SIG_MIN), LOG_SIG_MAX);
    const float sg = expf(ls), lsg = logf(sg);
    e += 0.5f + HALF_LOG_2PI + lsg;
    if (i == 0) logstd_c[a] = ls;
    if (i < n) {
      const float mu = meanp[(int64_t)i * OUT_LD + a];
      mean[(int64_t)i * A + a] = mu;
      stdv[(int64_t)i * A + a] = sg;
      if (acts != nullptr) {
        const float act = acts[(int64_t)i * A + a];
        const float x = !tanh_action ? act : (pre_tanh != nullptr ? pre_tanh[(int64_t)i * A + a] : tanh_pre(act));
        const float d = x - mu;
        lp += -(d * d) / (2.f * sg * sg) - lsg - HALF_LOG_2PI;
        if (tanh_action) lp -= tanh_corr(act);
      }
    }
  }
  if (i < n) {
    ent[i] = e;
    if (acts != nullptr) logp[i] = lp;
  }
}

// The same for GaussianContPolicy.forward (continuous_policy.py:222-236): `mean, log_std = x.chunk(2, -1)` of the padded head
// output outp [n][OUT_LD], log_std clamped and exponentiated per row: mean / std / clamped log_std [n][A], ent [n], log_prob [n].
__global__ __launch_bounds__(256) void gauss_head_sd_kernel(const float* __restrict__ outp, const float* __restrict__ acts, int n,
                                                            int A, float* __restrict__ mean, float* __restrict__ stdv,
                                                            float* __restrict__ logstd_c, float* __restrict__ ent,
                                                            float* __restrict__ logp, int tanh_action,
                                                            const float* __restrict__ pre_tanh) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float e = 0.f, lp = 0.f;
  for (int a = 0; a < A; ++a) {
    const float mu = outp[(int64_t)i * OUT_LD + a];
    const float ls = fminf(fmaxf(outp[(int64_t)i * OUT_LD + A + a], LOG_SIG_MIN), LOG_SIG_MAX);
    const float sg = expf(ls), lsg = logf(sg);
    e += 0.5f + HALF_LOG_2PI + lsg;
    mean[(int64_t)i * A + a] = mu;
    stdv[(int64_t)i * A + a] = sg;
    logstd_c[(int64_t)i * A + a] = ls;
    if (acts != nullptr) {
      const float act = acts[(int64_t)i * A + a];
      const float x = !tanh_action ? act : (pre_tanh != nullptr ? pre_tanh[(int64_t)i * A + a] : tanh_pre(act));
      const float d = x - mu;
      lp += -(d * d) / (2.f * sg * sg) - lsg - HALF_LOG_2PI;
      if (tanh_action) lp -= tanh_corr(act);
    }
  }
  ent[i] = e;
  if (acts != nullptr) logp[i] = lp;
}

// Categorical head post-processing for the policy API (CategoricalDisPolicy.forward / explore / update,
// policies/discrete_policies.py:136-172): from the padded logits [n][OUT_LD] the probabilities [n][K], the entropy [n] and, when
// acts != null, log_prob [n] of the action indices acts [n] (floats). gauss_head_kernel's counterpart.
__global__ __launch_bounds__(256) void cat_head_kernel(const float* __restrict__ logits, const float* __restrict__ acts, int n,
                                                       int K, float* __restrict__ probs, float* __restrict__ ent,
                                                       float* __restrict__ logp) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const CatDist d = cat_dist(logits + (int64_t)i * OUT_LD, K);
#pragma unroll
  for (int j = 0; j < CAT_CAP; ++j)
    if (j < K) probs[(int64_t)i * K + j] = d.p[j];
  ent[i] = d.ent;
  if (acts != nullptr) logp[i] = cat_logp(d, K, acts[i]);
}

// Copy column 0 of a padded head output to a contiguous [n] vector (critic values for the collector).
__global__ __launch_bounds__(256) void col0_kernel(const float* __restrict__ src, int n, float* __restrict__ dst) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[(int64_t)i * OUT_LD];
}

// --------------------------------------------------------------------------------- grad norm + Adam
// sum of squares of a flat gradient buffer -> part[blockIdx.x] (<= GRAD_NORM_PARTS blocks; clip_adam_kernel adds them in
// order). 16-byte loads, one or two per thread: the 388 K-float buffer is one short burst over the whole chip, not 24
// dependent trips of 64 blocks (12 us -> ~4 us).
constexpr int GRAD_NORM_PARTS = 256;
constexpr int ADAM_MAX_PARTS = 16384;  // partials clip_adam_kernel can add up (64 per thread; the NatureCNN nets have 9.4 K reduce blocks)
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ part) {
  double s = 0.0;
  const int64_t n4 = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 x = reinterpret_cast<const float4*>(g)[i];
    s += ((double)x.x * x.x + (double)x.y * x.y) + ((double)x.z * x.z + (double)x.w * x.w);
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n & 3)) { const float x = g[(n4 << 2) + threadIdx.x]; s += (double)x * x; }
  Red4 r = block_red4(s, 0.0, 0.f, 0.f);
  if (threadIdx.x == 0) part[blockIdx.x] = (float)r.s;
}

// One (tensor) segment of an optimiser's parameter set: parameters live in caller-owned tensors (pointer
// table), gradients and both Adam moments in flat buffers at offset goff.
struct ParamSeg { float* p; int64_t goff; int64_t n; int64_t blk0; };  // blk0: first block of this segment

// torch.nn.utils.clip_grad_norm_(params, max_norm) followed by torch.optim.Adam (eps after sqrt(v_hat),
// no weight decay == AdamW with wd 0) — torchrl/algo/on_policy/ppo.py:73-75,118-120, a2c.py:30-40.
// Operation order follows torch/optim/adam.py::_single_tensor_adam. The clip coefficient is derived from the
// squared norm accumulated in *sumsq; thread 0 of block 0 also publishes the pre-clip norm to *norm_out.
// Device-resident control block of the update loop. Everything that changes from one minibatch update to the
// next (which rows, Adam's bias corrections, where the statistics go) lives here and is advanced by kernels, so
// the launch sequence of an update is *identical* every time and can be replayed as one hipGraph.
struct UpdCtl {
  int upd_index;        // minibatch number inside the epoch: row of rowidx_all / stats_all
  int pad0;
  long long step[2];    // Adam steps committed so far for [0] pf, [1] vf: both advance once per update unless a guarded run
                        // (skip_all != null) skipped one optimiser's step — then that optimiser's count stays (GradScaler.step)
  double lr_pf, lr_vf;
  float beta1, beta2;
  float step_size[2];   // lr / (1 - beta1^(step+1)) for [0] pf, [1] vf — refreshed by upd_begin_body (block 0 of begin_pack_kernel)
  float bc2_sqrt[2];    // sqrt(1 - beta2^(step+1)), per optimiser
  double weight_decay;  // v4l_ppo_hyper.weight_decay (0: plain Adam), fixed for a run of updates
  float wd32;           // the same as torch hands it to grad.add(param, alpha=weight_decay) on fp32 tensors
  int decoupled;        // != 0: AdamW (decay the parameter), 0: L2 (decay joins the gradient)
  float decay[2];       // decoupled: 1 - lr * weight_decay per optimiser, formed in double and rounded once like step_size
  int kl_stop;          // the KL early stop's latch: cleared by v4l_trainer_kl_stop when it arms a run (kl_arm_kernel), set by
                        // kl_stop_kernel, read by clip_adam_kernel<WD, true> only — no other kernel touches the word
};
static_assert(sizeof(UpdCtl) <= 256, "UpdCtl must fit in front of stats_cur (control buffer layout [UpdCtl | stats_cur | rowidx_cur])");
__global__ void ctl_set_kernel(UpdCtl* c, int upd_index, long long step_pf, long long step_vf, double lr_pf, double lr_vf, float b1,
                               float b2, double weight_decay, int decoupled) {
  c->upd_index = upd_index; c->step[0] = step_pf; c->step[1] = step_vf; c->lr_pf = lr_pf; c->lr_vf = lr_vf; c->beta1 = b1; c->beta2 = b2;
  c->weight_decay = weight_decay; c->wd32 = (float)weight_decay; c->decoupled = decoupled; c->decay[0] = 1.f; c->decay[1] = 1.f;
}
__global__ void kl_arm_kernel(UpdCtl* c) { c->kl_stop = 0; }
// the candidate Adam step sizes / bias corrections of the update being opened, from the committed counts + 1 (double precision,
// like torch/optim/adam.py::_single_tensor_adam). Nothing is committed here: block 0 of each optimiser's clip_adam_kernel
// advances that optimiser's count when its step is taken.
__device__ __forceinline__ void upd_begin_step(UpdCtl* c) {
  if (threadIdx.x == 0) {
    const long long s0 = c->step[0] + 1, s1 = c->step[1] + 1;
    const double b1 = (double)c->beta1, b2 = (double)c->beta2;
    const double bc1 = 1.0 - pow(b1, (double)s0);
    const double bc2 = 1.0 - pow(b2, (double)s0);
    c->step_size[0] = (float)(c->lr_pf / bc1);
    c->bc2_sqrt[0] = (float)sqrt(bc2);
    if (s1 == s0) {  // the counts agree (always, unless a guarded run skipped a step): one pair of pow()s
      c->step_size[1] = (float)(c->lr_vf / bc1);
      c->bc2_sqrt[1] = c->bc2_sqrt[0];
    } else {
      c->step_size[1] = (float)(c->lr_vf / (1.0 - pow(b1, (double)s1)));
      c->bc2_sqrt[1] = (float)sqrt(1.0 - pow(b2, (double)s1));
    }
    if (c->decoupled) {  // AdamW: param.mul_(1 - lr * weight_decay) with this update's learning rates (adam.py:419)
      const double wd = c->weight_decay;
      c->decay[0] = (float)(1.0 - c->lr_pf * wd);
      c->decay[1] = (float)(1.0 - c->lr_vf * wd);
    }
  }
}
// Opens update #upd_index: selects its rows (identity when rowidx_all is null), clears the statistics record and
// computes the candidate Adam step sizes / bias corrections.
// adv != null: also the advantage statistics of the selected rows (adv_stats_kernel's work, one launch less).
__device__ __forceinline__ void upd_begin_body(UpdCtl* c, const int* __restrict__ rowidx_all, int n, int* rowidx_cur,
                                               float* stats_cur, const float* __restrict__ adv) {
  const int u = c->upd_index;
  if (adv != nullptr && n <= 4 * (int)blockDim.x) {
    // (round 5) the rows' indices and advantages stay in registers: index -> advantage is the only dependent pair of round
    // trips left in this block's chain (it was index -> store -> barrier -> reload -> advantage -> second pass)
    int ri[4];
    float av[4];
    bool ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = (int)threadIdx.x + j * (int)blockDim.x;
      ok[j] = i < n;
      ri[j] = rowidx_all ? rowidx_all[(int64_t)u * n + (ok[j] ? i : 0)] : i;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) av[j] = adv[ok[j] ? ri[j] : 0];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (ok[j]) rowidx_cur[(int)threadIdx.x + j * (int)blockDim.x] = ri[j];
    if (threadIdx.x < ST_SIZE) stats_cur[threadIdx.x] = 0.f;
    upd_begin_step(c);  // (thread 0's double-precision pow() runs while the loads above are in flight)
    __syncthreads();  // the cleared record is in place before thread 0 fills its part
    adv_stats_regs(av, ok, n, stats_cur);
    return;
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x) rowidx_cur[i] = rowidx_all ? rowidx_all[(int64_t)u * n + i] : i;
    if (threadIdx.x < ST_SIZE) stats_cur[threadIdx.x] = 0.f;
    if (adv != nullptr) {
      __syncthreads();  // rowidx_cur and the cleared record are visible to the whole block
      adv_stats_body(adv, rowidx_cur, n, stats_cur);
    }
  }
  upd_begin_step(c);
}
// WD: how v4l_ppo_hyper.weight_decay enters (a template argument: without decay the launch is the kernel it always was).
//   WD_NONE       no decay
//   WD_COUPLED    torch.optim.Adam(weight_decay=wd): grad = grad.add(param, alpha=wd) on the clipped gradient, before both moments
//   WD_DECOUPLED  torch.optim.AdamW: param.mul_(1 - lr * wd), then the plain step on the decayed parameter
// The norm (and the logged grad_norm) is the raw gradient's either way: clip_grad_norm_ runs before optimizer.step().
enum { WD_NONE = 0, WD_COUPLED = 1, WD_DECOUPLED = 2 };
// KL: the launch belongs to a run with the KL early stop armed (v4l_trainer_kl_update_*). A template argument like WD, same
// signature: the instantiation every other run launches, clip_adam_kernel<WD>, has neither the load nor the test.
template <int WD, bool KL = false>
__global__ __launch_bounds__(256) void clip_adam_kernel(const ParamSeg* __restrict__ segs, int nseg,
                                                        const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, const float* __restrict__ part, int npart,
                                                        const float* __restrict__ extra, int nextra, float max_norm, float eps, UpdCtl* ctl,
                                                        int which, float* __restrict__ norm_out, UpdCtl* close_ctl,
                                                        const float* stats_cur, float* __restrict__ stats_all, int* __restrict__ skip_all,
                                                        unsigned nf_exempt) {
  const ParamSeg sg = segs[find_desc(segs, nseg, (int64_t)blockIdx.x)];
  const float beta1 = ctl->beta1, beta2 = ctl->beta2;
  const float step_size = ctl->step_size[which], bc2_sqrt = ctl->bc2_sqrt[which];
  const float wd = WD == WD_COUPLED ? ctl->wd32 : WD == WD_DECOUPLED ? ctl->decay[which] : 0.f;  // (no load for WD_NONE)
  const int lane_ = threadIdx.x & 63;
  // this thread's element: its four operands are requested before the norm is summed (they do not depend on it; behind the
  // barrier below they would be one more round trip at the end of the block's chain — round 5)
  const int64_t i = ((int64_t)blockIdx.x - sg.blk0) * 256 + threadIdx.x;
  const bool mine = i < sg.n;
  const int64_t o = sg.goff + (mine ? i : 0);
  const float g_in = g[o], m_in = m[o], v_in = v[o], p_in = sg.p[mine ? i : 0];
  // the norm's partials (grad_sumsq_kernel's, or one per wgrad_reduce block: npart <= ADAM_MAX_PARTS), strided over the block's
  // threads with every load in flight at once, then lanes -> waves in a fixed order: the same bits in every block
  __shared__ float wpart[4];
  float pv[ADAM_MAX_PARTS / 256];
#pragma unroll
  for (int i = 0; i < ADAM_MAX_PARTS / 256; ++i) {
    const int k = (int)threadIdx.x + 256 * i;
    pv[i] = part[k < npart ? k : 0];
  }
  float ps = 0.f;
#pragma unroll
  for (int i = 0; i < ADAM_MAX_PARTS / 256; ++i) ps += (int)threadIdx.x + 256 * i < npart ? pv[i] : 0.f;
  if ((int)threadIdx.x < nextra) { const float x = extra[threadIdx.x]; ps = fmaf(x, x, ps); }  // gradients no reduce block wrote (log sigma)
  ps = wave_sum(ps);
  if (lane_ == 0) wpart[threadIdx.x >> 6] = ps;
  __syncthreads();
  const float tot = sqrtf((wpart[0] + wpart[1]) + (wpart[2] + wpart[3]));
  const float coef = fminf(max_norm / (tot + 1e-6f), 1.f);
  if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out != nullptr) *norm_out = tot;
  // skip_all != null (the opt-in guard): a step whose pre-clip norm is not finite writes nothing and does not count. Every block
  // summed the same partials in the same order, so every block takes the same decision without a grid-wide sync (data parallel:
  // the partials are those of the all-reduced bucket, so every rank skips the same steps).
  const bool nonfinite = skip_all != nullptr && !(fabsf(tot) <= 3.0e38f);
  // KL: a set latch skips the step the same way. The latch was written by an earlier launch on this stream (kl_stop_kernel) and
  // no launch writes it while this one runs: every block reads the same word.
  bool skip = nonfinite;
  if (KL) skip = skip || ctl->kl_stop != 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (!skip) ctl->step[which] = ctl->step[which] + 1;  // commit this optimiser's Adam step
    // (the update index before the closing block below advances it: program order of this thread)
    if (skip_all != nullptr) skip_all[(int64_t)ctl->upd_index * 2 + which] = nonfinite ? 1 : 0;  // "non-finite" only, never the KL stop
  }
  if (blockIdx.x == 0 && close_ctl != nullptr) {
    // last launch of an update: publish the statistics record (this block just completed it with the policy's gradient
    // norm) and move on to the next minibatch (no separate closing launch)
    __syncthreads();
    const int u = close_ctl->upd_index;
    if (threadIdx.x < 64) {  // wave 0: count the non-finite logger scalars (losses, norms, ratios: a NaN anywhere reaches them)
      // nf_exempt: record slots whose NaN is the reference's own value, not a fault (log_std/std of a 1-dimensional action:
      // torch's std() of one element) — logged as NaN, not counted
      const float sv = threadIdx.x < 18 && !((nf_exempt >> threadIdx.x) & 1u) ? stats_cur[threadIdx.x] : 0.f;
      const unsigned long long badm = __ballot(!(fabsf(sv) <= 3.0e38f));
      if (threadIdx.x == 0) const_cast<float*>(stats_cur)[ST_NONFINITE] = (float)__popcll(badm);
    }
    __syncthreads();
    if (stats_all != nullptr && threadIdx.x < ST_SIZE) stats_all[(int64_t)u * ST_SIZE + threadIdx.x] = stats_cur[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) close_ctl->upd_index = u + 1;
  }
  if (!mine || skip) return;
  float gr = g_in * coef;
  float pp = p_in;
  if (WD == WD_COUPLED) gr = fmaf(wd, pp, gr);  // one rounding for clip_coef * g + wd * p's sum
  if (WD == WD_DECOUPLED) pp = pp * wd;
  float mm = m_in, vv = v_in;
  mm = mm + (gr - mm) * (1.f - beta1);           // exp_avg.lerp_(grad, 1 - beta1)
  vv = vv * beta2 + (1.f - beta2) * (gr * gr);   // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2)
  const float denom = sqrtf(vv) / bc2_sqrt + eps;
  sg.p[i] = pp - step_size * (mm / denom);       // param.addcdiv_(exp_avg, denom, value=-step_size)
  m[o] = mm;
  v[o] = vv;
}

#pragma clang fp contract(on)  // (per-statement contraction, as for the PPO loss rows above)
// --------------------------------------------------------------------------------- V-MPO (torchrl/algo/on_policy/v_mpo.py)
// VMPO.update_actor's `torch.sort(advs, descending=True)` + `idx.chunk(2)` (v_mpo.py:65-67) by counting: sel[r] = the rollout
// slot of the minibatch row with the r-th largest advantage, r < m = ceil(n / 2). One thread per row, the n advantages staged
// through LDS 256 at a time (every lane reads the same LDS words: a broadcast), rank_i = #{j : adv_j > adv_i or (adv_j == adv_i
// and j < i)}: a strict total order, so the ranks are a permutation of 0 .. n-1 and every sel entry has exactly one writer — no
// atomics, the same output every run. Ties go to the earlier minibatch position (torch leaves their order unspecified); a NaN
// compares as smaller than every number (NaNs among themselves by position), so sel is written whole and in bounds whatever
// the advantages hold. rowidx null: row i is slot i.
// The order as one integer compare: the float mapped monotonically to an unsigned (NaN -> 0, below -inf's image; -0 == +0) in the
// high word, 0x7fffffff - position in the low one — key_j > key_i <=> row j sorts before row i. 0 is no row's key (padding).
__device__ __forceinline__ unsigned long long vmpo_key(float a, int j) {
  const unsigned u = a == 0.f ? 0u : __float_as_uint(a);
  const unsigned k = a != a ? 0u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
  return ((unsigned long long)k << 32) | (unsigned)(0x7fffffff - j);
}
__global__ __launch_bounds__(256) void vmpo_select_kernel(const float* __restrict__ adv, const int* __restrict__ rowidx, int n,
                                                          int* __restrict__ sel) {
  __shared__ __align__(16) unsigned long long tile[256];
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  const bool mine = i < n;
  const int slot = mine ? (rowidx ? rowidx[i] : i) : 0;
  const unsigned long long ki = vmpo_key(mine ? adv[slot] : 0.f, i);
  int rank = 0;
  for (int t0 = 0; t0 < n; t0 += 256) {
    const int j = t0 + (int)threadIdx.x;
    const unsigned long long kj = j < n ? vmpo_key(adv[rowidx ? rowidx[j] : j], j) : 0ull;
    __syncthreads();  // the previous tile has been read by every thread
    tile[threadIdx.x] = kj;
    __syncthreads();
    const ulonglong2* t2 = reinterpret_cast<const ulonglong2*>(tile);  // 16-byte LDS reads, several in flight
#pragma unroll 8
    for (int k = 0; k < 128; ++k) {
      const ulonglong2 v = t2[k];
      rank += (v.x > ki ? 1 : 0) + (v.y > ki ? 1 : 0);
    }
  }
  const int m = (n + 1) / 2;
  if (mine && rank < m) sel[rank] = slot;
}

// The two learnable scalars of V-MPO (eta: temperature of the advantage softmax, alpha: weight of the KL term; v_mpo.py:27-39)
// with the state of their optimiser, `optimizer_class([eta, alpha], lr=plr, eps=1e-5)`: one device block the trainer owns.
struct VmpoState { double eta, alpha, m[2], v[2]; long long step; };  // m / v: Adam moments of [0] eta, [1] alpha
// V4L_VMPO_STATS floats per update, next to the PPO record: the seven logger scalars V-MPO adds (v_mpo.py:119-132) and the two
// scalar gradients (diagnostic)
enum { VST_ALPHA_LOSS = 0, VST_ALPHA, VST_ETA, VST_KL_MEAN, VST_KL_STD, VST_KL_MAX, VST_KL_MIN, VST_DETA, VST_DALPHA, VST_SIZE = 12 };
struct VmpoArgs {
  VmpoState* vs;
  float *vst_cur, *vst_all;  // the record being filled; [U][VST_SIZE] records of the run (row ctl->upd_index) or null
  const UpdCtl* ctl;         // lr_pf, betas, weight decay of the open run
  double eta_eps, alpha_eps;
  double lr_scale;           // 1; 0 leaves eta, alpha and their optimiser state untouched (tests look at the gradients alone)
  float adam_eps;
};
// VMPO.update_actor's loss (v_mpo.py:75-102) on the m selected rows (p.rowidx = sel, p.n = m, p.inv_n = 1 / m) and its gradient
// w.r.t. the policy mean [m][OUT_LD], log sigma [A], eta and alpha; single block, the sibling of actor_loss_kernel.
//   phis = softmax(an / eta)                       an: the advantage normalised with the WHOLE minibatch's statistics (p.st)
//   policy_loss = mean_i(-phis_i logp_i + alpha kl_i)       kl_i = sum_a KL(N(mu, sigma) || N(mu_t, sigma_t)): plain Normals also
//                                                           for tanh_action policies (continuous_policy.py:127-146)
//   eta_loss = eta eta_eps + eta log(mean(exp(an / eta)))   alpha_loss = alpha alpha_eps - alpha mean(kl)
// Pass 1: max and sum of exp(an / eta - max) (the reference does not subtract the max; the same value while it does not
// overflow). Pass 2: the rows. Thread 0 then takes the Adam / AdamW step of the two scalars in double, clamps them at 1e-8
// (v_mpo.py:113-117) and files the V-MPO record. Fills the PPO record's shared slots as actor_loss_body does (ratio =
// exp(logp - logp_target)), so the closing Adam launch's non-finite count works unchanged.
template <bool TANH, int CAP>
__global__ __launch_bounds__(1024) void vmpo_loss_kernel(ActorArgs p, VmpoArgs q) {
  __shared__ float sdl[16][CAP];
  const int m = p.n, A = p.A;
  const ActorDimsT<CAP> D = actor_dims<CAP>(p);
  float dl[CAP];
#pragma unroll
  for (int a = 0; a < CAP; ++a) dl[a] = 0.f;
  const float amean = p.st[ST_ADV_MEAN], astd = p.st[ST_ADV_STD];
  const double eta_d = q.vs->eta, alpha_d = q.vs->alpha;
  const float eta = (float)eta_d, alpha = (float)alpha_d;
  // the thread's first row (its only one while m <= blockDim.x): slot and normalised advantage stay in registers over the passes
  const int i0 = (int)threadIdx.x;
  const int slot0 = i0 < m ? p.rowidx[i0] : 0;
  const float an0 = i0 < m ? (p.adv[slot0] - amean) / (astd + 1e-5f) : 0.f;
  // ---- pass 1
  float xmx = -INFINITY;
  for (int i = threadIdx.x; i < m; i += blockDim.x) {
    const float an = i == i0 ? an0 : (p.adv[p.rowidx[i]] - amean) / (astd + 1e-5f);
    xmx = fmaxf(xmx, an / eta);
  }
  const float xmax = block_red4(0.0, 0.0, xmx, 0.f).mx;
  double se = 0.0, sea = 0.0;
  for (int i = threadIdx.x; i < m; i += blockDim.x) {
    const float an = i == i0 ? an0 : (p.adv[p.rowidx[i]] - amean) / (astd + 1e-5f);
    const float e = expf(an / eta - xmax);
    se += e; sea += (double)e * an;
  }
  const Red4 r0 = block_red4(se, sea, 0.f, 0.f);
  const float esum = (float)r0.s;
  // ---- pass 2
  double s_lp = 0.0, s_lp2 = 0.0, s_kl = 0.0, s_kl2 = 0.0, s_loss = 0.0;
  int sat = 0;
  float lp_mx = -INFINITY, lp_mn = INFINITY, kl_mx = -INFINITY, kl_mn = INFINITY, r_mx = -INFINITY, r_mn = INFINITY;
  for (int i = threadIdx.x; i < m; i += blockDim.x) {
    const int slot = i == i0 ? slot0 : p.rowidx[i];
    const float an = i == i0 ? an0 : (p.adv[slot] - amean) / (astd + 1e-5f);
    const float phi = expf(an / eta - xmax) / esum;
    float mu[CAP], tmu[CAP], dmr[CAP];
    actor_load_row(p.mean + (int64_t)i * OUT_LD, mu);
    actor_load_row(p.tmean + (int64_t)i * OUT_LD, tmu);
    float lp = 0.f, lpt = 0.f, kl = 0.f;
#pragma unroll
    for (int a = 0; a < CAP; ++a) {
      dmr[a] = 0.f;
      if (a < A) {
        const float act = p.acts[(int64_t)slot * A + a];
        const float x = TANH ? tanh_pre(act) : act;
        const float corr = TANH ? tanh_corr(act) : 0.f;
        const float d = x - mu[a], dt = x - tmu[a], dmu = mu[a] - tmu[a];
        const float var = D.sg[a] * D.sg[a], tvar = D.tsg[a] * D.tsg[a];
        lp += -(d * d) / (2.f * var) - D.lsg[a] - HALF_LOG_2PI - corr;
        lpt += -(dt * dt) / (2.f * tvar) - D.tlsg[a] - HALF_LOG_2PI - corr;
        // torch.distributions.kl._kl_normal_normal: 0.5 (var_ratio + t1 - 1 - log(var_ratio))
        const float sr = D.sg[a] / D.tsg[a], vr = sr * sr, t1 = (dmu / D.tsg[a]) * (dmu / D.tsg[a]);
        kl += 0.5f * (vr + t1 - 1.f - logf(vr));
        dmr[a] = grad_out(p.inv_n * (-phi * (d / var) + alpha * (dmu / tvar)), p.gscale, sat);
        dl[a] += p.inv_n * (-phi * (d * d / var - 1.f) + alpha * (vr - 1.f));
      }
    }
    actor_store_dmean(p.dmean + (int64_t)i * OUT_LD, dmr, true);
    const float ratio = expf(lp - lpt);
    s_loss += (double)(-phi * lp + alpha * kl);
    s_lp += lp; s_lp2 += (double)lp * lp;
    s_kl += kl; s_kl2 += (double)kl * kl;
    lp_mx = fmaxf(lp_mx, lp); lp_mn = fminf(lp_mn, lp);
    kl_mx = fmaxf(kl_mx, kl); kl_mn = fminf(kl_mn, kl);
    r_mx = fmaxf(r_mx, ratio); r_mn = fminf(r_mn, ratio);
  }
  const Red4 r1 = block_red4(s_lp, s_lp2, lp_mx, lp_mn);
  const Red4 r2 = block_red4(s_kl, s_kl2, kl_mx, kl_mn);
  const Red4 r3 = block_red4(s_loss, (double)sat, r_mx, r_mn);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < CAP; ++a) {
    const float v = wave_sum(dl[a]);
    if (lane == 0) sdl[w][a] = v;
  }
  __syncthreads();
  if (threadIdx.x < A) {
    const int a = threadIdx.x;
    const float raw = p.logstd[a];
    float g = 0.f;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) g += sdl[k][a];
    p.dlogstd[a] = (raw >= LOG_SIG_MIN && raw <= LOG_SIG_MAX) ? g : 0.f;  // the clamp of continuous_policy.py:486-492 passes no gradient outside
  }
  if (threadIdx.x == 0) {
    float* st = p.st;
    const double dm = (double)m;
    const double lpm = r1.s / dm, klm = r2.s / dm;
    st[ST_PI_LOSS] = (float)(r3.s / dm);
    st[ST_LP_MEAN] = (float)lpm;
    st[ST_LP_STD] = (float)sqrt(fmax(0.0, (r1.s2 - dm * lpm * lpm) / (dm - 1.0)));
    st[ST_LP_MAX] = r1.mx; st[ST_LP_MIN] = r1.mn;
    st[ST_RATIO_MAX] = r3.mx; st[ST_RATIO_MIN] = r3.mn;
    if (p.gscale != 1.f) st[ST_F16_SAT] += (float)r3.s2;
    double lm = 0.0; float lmx = -INFINITY, lmn = INFINITY;
#pragma unroll
    for (int a = 0; a < CAP; ++a)
      if (a < A) { lm += D.ls[a]; lmx = fmaxf(lmx, D.ls[a]); lmn = fminf(lmn, D.ls[a]); }
    lm /= A;
    double lq = 0.0;
#pragma unroll
    for (int a = 0; a < CAP; ++a)
      if (a < A) lq += (D.ls[a] - lm) * (D.ls[a] - lm);
    st[ST_LS_MEAN] = (float)lm;
    st[ST_LS_STD] = A > 1 ? (float)sqrt(lq / (A - 1)) : NAN;
    st[ST_LS_MAX] = lmx; st[ST_LS_MIN] = lmn;
    // d(eta_loss)/d(eta) = eta_eps + log(mean(exp(an / eta))) - (sum_i phis_i an_i) / eta;  d(alpha_loss)/d(alpha) = alpha_eps - mean(kl)
    const double lme = (double)xmax + log(r0.s / dm);
    const double grad[2] = {q.eta_eps + lme - (r0.s2 / r0.s) / eta_d, q.alpha_eps - klm};
    VmpoState s = *q.vs;
    double par[2] = {s.eta, s.alpha};
    if (q.lr_scale != 0.0) {
      // torch/optim/adam.py::_single_tensor_adam on two one-element tensors, in double; the parameters are kept as the fp32
      // values the reference's tensors would hold
      const double lr = q.ctl->lr_pf * q.lr_scale, b1 = (double)q.ctl->beta1, b2 = (double)q.ctl->beta2;
      const double wd = q.ctl->weight_decay;
      s.step += 1;
      const double bc1 = 1.0 - pow(b1, (double)s.step), bc2 = 1.0 - pow(b2, (double)s.step);
      for (int k = 0; k < 2; ++k) {
        double g = grad[k], pp = par[k];
        if (wd > 0.0 && q.ctl->decoupled) pp *= 1.0 - lr * wd;
        if (wd > 0.0 && !q.ctl->decoupled) g += wd * pp;
        s.m[k] += (g - s.m[k]) * (1.0 - b1);
        s.v[k] = s.v[k] * b2 + (1.0 - b2) * g * g;
        pp -= (lr / bc1) * (s.m[k] / (sqrt(s.v[k]) / sqrt(bc2) + (double)q.adam_eps));
        par[k] = (double)(float)fmax(pp, 1e-8);  // torch.clamp(min=1e-8), v_mpo.py:115-117 (a NaN stays a NaN)
      }
      s.eta = par[0]; s.alpha = par[1];
      *q.vs = s;
    }
    float rec[VST_SIZE];
#pragma unroll
    for (int k = 0; k < VST_SIZE; ++k) rec[k] = 0.f;
    rec[VST_ALPHA_LOSS] = (float)(alpha_d * q.alpha_eps - alpha_d * klm);  // with the alpha the loss was formed with
    rec[VST_ALPHA] = (float)par[1]; rec[VST_ETA] = (float)par[0];       // after the step and the clamp (v_mpo.py:121-122)
    rec[VST_KL_MEAN] = (float)klm;
    rec[VST_KL_STD] = (float)sqrt(fmax(0.0, (r2.s2 - dm * klm * klm) / (dm - 1.0)));
    rec[VST_KL_MAX] = r2.mx; rec[VST_KL_MIN] = r2.mn;
    rec[VST_DETA] = (float)grad[0]; rec[VST_DALPHA] = (float)grad[1];
    const int64_t u = q.ctl->upd_index;
#pragma unroll
    for (int k = 0; k < VST_SIZE; ++k) {
      q.vst_cur[k] = rec[k];
      if (q.vst_all != nullptr) q.vst_all[u * VST_SIZE + k] = rec[k];
    }
  }
}
__global__ void vmpo_state_set_kernel(VmpoState* vs, double eta, double alpha, double m0, double m1, double v0, double v1, long long step) {
  vs->eta = eta; vs->alpha = alpha; vs->m[0] = m0; vs->m[1] = m1; vs->v[0] = v0; vs->v[1] = v1; vs->step = step;
}

// --------------------------------------------------------------------------------- A2C (torchrl/algo/on_policy/a2c.py)
// V4L_A2C_STATS floats per update, next to the PPO record: the 12 logger scalars of A2C.update in the reference's order
// (a2c.py:89-105). The critic's loss launch files AST_VF_LOSS .. AST_VP_MIN, the policy's the rest, both in row ctl->upd_index.
enum { AST_PI_LOSS = 0, AST_VF_LOSS, AST_VP_MEAN, AST_VP_STD, AST_VP_MAX, AST_VP_MIN, AST_SD_MEAN, AST_SD_STD, AST_SD_MAX, AST_SD_MIN,
       AST_ENT, AST_LOGP, AST_SIZE = V4L_A2C_STATS };
static_assert(AST_LOGP < AST_SIZE, "the A2C record holds the 12 keys");
// nn.MSELoss()(vf(obs), est_rets) and its gradient (a2c.py:76-77): critic_loss_body with clipped = 0, then values.mean(), .std()
// (Bessel), .max(), .min() of the critic's output column (a2c.py:92-95). Single block.
__global__ __launch_bounds__(1024) void a2c_critic_loss_kernel(const float* __restrict__ values, const float* __restrict__ ret,
                                                              const int* __restrict__ rowidx, int n, float inv_n,
                                                              float* __restrict__ dvalues, float* __restrict__ st, float gscale,
                                                              const UpdCtl* __restrict__ ctl, float* __restrict__ ast_all) {
  critic_loss_body(values, ret, nullptr, rowidx, n, inv_n, 0, 0.f, dvalues, st, gscale);
  double s = 0.0; float mx = -INFINITY, mn = INFINITY;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float v = values[(int64_t)i * OUT_LD];
    s += v; mx = fmaxf(mx, v); mn = fminf(mn, v);
  }
  const Red4 r = block_red4(s, 0.0, mx, mn);
  const double mean = r.s / n;
  double q = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const double v = values[(int64_t)i * OUT_LD];
    q += (v - mean) * (v - mean);
  }
  const Red4 r2 = block_red4(q, 0.0, 0.f, 0.f);
  if (threadIdx.x == 0) {
    float* ast = ast_all + (int64_t)ctl->upd_index * AST_SIZE;
    ast[AST_VF_LOSS] = st[ST_VF_LOSS];  // (this thread wrote it in critic_loss_body)
    ast[AST_VP_MEAN] = (float)mean;
    ast[AST_VP_STD] = (float)sqrt(r2.s / (double)(n - 1));
    ast[AST_VP_MAX] = r.mx; ast[AST_VP_MIN] = r.mn;
  }
}
// A2C.update's policy loss (a2c.py:61-74) and its gradient w.r.t. the policy mean [n][OUT_LD] and log sigma [A]; single block,
// the sibling of actor_loss_kernel without ratio, clip or target policy (p.tmean, p.tlogstd, p.logp_old, p.clip unused).
//   policy_loss = mean_i(-logp_i an_i) - ent_coef ent        an: the advantage normalised with the minibatch statistics in p.st
//   ent = sum_a (0.5 + 0.5 log(2 pi) + log sigma_a): the plain Normal's also for TanhNormal policies (distribution.py:79-80),
//   the same for every row, so ent.mean() is that sum.
// std/*: over the [n][A] expanded tensor pf.update returns (continuous_policy.py:252-253): every column holds one sigma n times.
// Fills ST_PI_LOSS and ST_LP_MEAN of the PPO record (the closing Adam launch's non-finite count reads them); the record's other
// policy slots stay at the cleared 0.
template <bool TANH, int CAP>
__global__ __launch_bounds__(1024) void a2c_loss_kernel(ActorArgs p, const UpdCtl* __restrict__ ctl, float* __restrict__ ast_all) {
  __shared__ float sdl[16][CAP];
  const int n = p.n, A = p.A;
  const ActorDimsT<CAP> D = actor_dims<CAP>(p);
  float dl[CAP];
#pragma unroll
  for (int a = 0; a < CAP; ++a) dl[a] = 0.f;
  const float amean = p.st[ST_ADV_MEAN], astd = p.st[ST_ADV_STD];
  double s_lp = 0.0, s_loss = 0.0;
  int sat = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int slot = p.rowidx ? p.rowidx[i] : i;
    const float an = (p.adv[slot] - amean) / (astd + 1e-5f);
    const float dlp = -p.inv_n * an;  // d(mean(-logp an)) / d(logp_i)
    float mu[CAP], dmr[CAP];
    actor_load_row(p.mean + (int64_t)i * OUT_LD, mu);
    float lp = 0.f;
#pragma unroll
    for (int a = 0; a < CAP; ++a) {
      dmr[a] = 0.f;
      if (a < A) {
        const float act = p.acts[(int64_t)slot * A + a];
        const float x = TANH ? tanh_pre(act) : act;
        const float corr = TANH ? tanh_corr(act) : 0.f;
        const float d = x - mu[a];
        const float var = D.sg[a] * D.sg[a];
        lp += -(d * d) / (2.f * var) - D.lsg[a] - HALF_LOG_2PI - corr;
        dmr[a] = grad_out(dlp * (d / var), p.gscale, sat);
        dl[a] += dlp * (d * d / var - 1.f);
      }
    }
    actor_store_dmean(p.dmean + (int64_t)i * OUT_LD, dmr, true);
    s_loss += (double)(-lp * an);
    s_lp += lp;
  }
  const Red4 r = block_red4(s_loss, s_lp, 0.f, 0.f);
  const Red4 r2 = block_red4((double)sat, 0.0, 0.f, 0.f);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < CAP; ++a) {
    const float v = wave_sum(dl[a]);
    if (lane == 0) sdl[w][a] = v;
  }
  __syncthreads();
  if (threadIdx.x < A) {
    const int a = threadIdx.x;
    const float raw = p.logstd[a];
    float g = 0.f;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) g += sdl[k][a];
    g += -p.ent_coef * p.inv_n * (float)n;  // the entropy term, as in actor_loss_body
    p.dlogstd[a] = (raw >= LOG_SIG_MIN && raw <= LOG_SIG_MAX) ? g : 0.f;  // the clamp of continuous_policy.py:486-492 passes no gradient outside
  }
  if (threadIdx.x == 0) {
    float* st = p.st;
    const double lpm = r.s2 / n;
    const float loss = (float)(r.s / n - (double)p.ent_coef * D.ent);
    st[ST_PI_LOSS] = loss;
    st[ST_LP_MEAN] = (float)lpm;
    if (p.gscale != 1.f) st[ST_F16_SAT] += (float)r2.s;
    double m = 0.0; float mx = -INFINITY, mn = INFINITY;
#pragma unroll
    for (int a = 0; a < CAP; ++a)
      if (a < A) { m += D.sg[a]; mx = fmaxf(mx, D.sg[a]); mn = fminf(mn, D.sg[a]); }
    m /= A;
    double q = 0.0;
#pragma unroll
    for (int a = 0; a < CAP; ++a)
      if (a < A) q += (D.sg[a] - m) * (D.sg[a] - m);
    const double cnt = (double)n * A;  // (n >= 2: never one element)
    float* ast = ast_all + (int64_t)ctl->upd_index * AST_SIZE;
    ast[AST_PI_LOSS] = loss;
    ast[AST_SD_MEAN] = (float)m;
    ast[AST_SD_STD] = (float)sqrt((double)n * q / (cnt - 1.0));
    ast[AST_SD_MAX] = mx; ast[AST_SD_MIN] = mn;
    ast[AST_ENT] = D.ent;
    ast[AST_LOGP] = (float)lpm;
  }
}

// --------------------------------------------------------------------------------- REINFORCE (torchrl/algo/on_policy/reinforce.py)
// V4L_REINFORCE_STATS floats per update, next to the PPO record: the 10 logger scalars of Reinforce.update in the reference's
// order (reinforce.py:43-74); slots 10, 11 stay as the caller cleared them.
enum { RST_ADV_MEAN = 0, RST_ADV_STD, RST_ADV_MAX, RST_ADV_MIN, RST_PI_LOSS, RST_ENT, RST_LP_MEAN, RST_LP_STD, RST_LP_MAX, RST_LP_MIN,
       RST_SIZE = V4L_REINFORCE_STATS };
static_assert(RST_LP_MIN < RST_SIZE, "the REINFORCE record holds the 10 keys");
// Reinforce.update's policy loss (reinforce.py:52-61) and its gradient w.r.t. the policy mean [n][OUT_LD] and log sigma [A];
// single block, the sibling of a2c_loss_kernel: the same rows, the same log sigma reduction with the entropy term and the clamp
// gate, and on top of it logprob/std (Bessel), max, min (reinforce.py:69-72). No critic, so no std/* of A2C's record; advs/mean,
// max and min are copied from the PPO record, where the opening launch left them, advs/std is formed from its M2 slot.
//   policy_loss = mean_i(-logp_i an_i) - ent_coef ent        an: the advantage normalised with the minibatch statistics in p.st
//   ent = sum_a (0.5 + 0.5 log(2 pi) + log sigma_a): the plain Normal's also for TanhNormal policies (distribution.py:79-80)
// Fills ST_PI_LOSS and ST_LP_MEAN / STD / MAX / MIN of the PPO record (the closing Adam launch's non-finite count reads them); its
// ST_LS_* and ST_RATIO_* stay at the cleared 0. A sibling, not a shared body: a2c_loss_kernel reduces two sums and no extrema,
// and its instantiations stay the code they were.
template <bool TANH, int CAP>
__global__ __launch_bounds__(1024) void reinforce_loss_kernel(ActorArgs p, const UpdCtl* __restrict__ ctl, float* __restrict__ rst_all) {
  __shared__ float sdl[16][CAP];
  const int n = p.n, A = p.A;
  const ActorDimsT<CAP> D = actor_dims<CAP>(p);
  float dl[CAP];
#pragma unroll
  for (int a = 0; a < CAP; ++a) dl[a] = 0.f;
  const float amean = p.st[ST_ADV_MEAN], astd = p.st[ST_ADV_STD];
  double s_lp = 0.0, s_lp2 = 0.0, s_loss = 0.0;
  float lp_mx = -INFINITY, lp_mn = INFINITY;
  int sat = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int slot = p.rowidx ? p.rowidx[i] : i;
    const float an = (p.adv[slot] - amean) / (astd + 1e-5f);
    const float dlp = -p.inv_n * an;  // d(mean(-logp an)) / d(logp_i)
    float mu[CAP], dmr[CAP];
    actor_load_row(p.mean + (int64_t)i * OUT_LD, mu);
    float lp = 0.f;
#pragma unroll
    for (int a = 0; a < CAP; ++a) {
      dmr[a] = 0.f;
      if (a < A) {
        const float act = p.acts[(int64_t)slot * A + a];
        const float x = TANH ? tanh_pre(act) : act;
        const float corr = TANH ? tanh_corr(act) : 0.f;
        const float d = x - mu[a];
        const float var = D.sg[a] * D.sg[a];
        lp += -(d * d) / (2.f * var) - D.lsg[a] - HALF_LOG_2PI - corr;
        dmr[a] = grad_out(dlp * (d / var), p.gscale, sat);
        dl[a] += dlp * (d * d / var - 1.f);
      }
    }
    actor_store_dmean(p.dmean + (int64_t)i * OUT_LD, dmr, true);
    s_loss += (double)(-lp * an);
    s_lp += lp; s_lp2 += (double)lp * lp;
    lp_mx = fmaxf(lp_mx, lp); lp_mn = fminf(lp_mn, lp);
  }
  const Red4 r = block_red4(s_lp, s_lp2, lp_mx, lp_mn);
  const Red4 r2 = block_red4(s_loss, (double)sat, 0.f, 0.f);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < CAP; ++a) {
    const float v = wave_sum(dl[a]);
    if (lane == 0) sdl[w][a] = v;
  }
  __syncthreads();
  if (threadIdx.x < A) {
    const int a = threadIdx.x;
    const float raw = p.logstd[a];
    float g = 0.f;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) g += sdl[k][a];
    g += -p.ent_coef * p.inv_n * (float)n;  // the entropy term, as in actor_loss_body
    p.dlogstd[a] = (raw >= LOG_SIG_MIN && raw <= LOG_SIG_MAX) ? g : 0.f;  // the clamp of continuous_policy.py:486-492 passes no gradient outside
  }
  if (threadIdx.x == 0) {
    float* st = p.st;
    const double dn = (double)n;
    const double lpm = r.s / dn;
    const float loss = (float)(r2.s / dn - (double)p.ent_coef * D.ent);
    const float lps = (float)sqrt(fmax(0.0, (r.s2 - dn * lpm * lpm) / (dn - 1.0)));  // (n >= 2: never one element)
    st[ST_PI_LOSS] = loss;
    st[ST_LP_MEAN] = (float)lpm;
    st[ST_LP_STD] = lps;
    st[ST_LP_MAX] = r.mx; st[ST_LP_MIN] = r.mn;
    if (p.gscale != 1.f) st[ST_F16_SAT] += (float)r2.s2;
    float* rst = rst_all + (int64_t)ctl->upd_index * RST_SIZE;
    // advs/std: the reference takes it from the numpy batch before the upload (reinforce.py:43-46), so it is numpy's std — the
    // population one, sqrt(M2 / n) — while the normalisation above uses torch's (Bessel) as reinforce.py:57 does
    rst[RST_ADV_MEAN] = st[ST_ADV_MEAN]; rst[RST_ADV_STD] = (float)sqrt((double)st[ST_ADV_M2] / dn);
    rst[RST_ADV_MAX] = st[ST_ADV_MAX]; rst[RST_ADV_MIN] = st[ST_ADV_MIN];
    rst[RST_PI_LOSS] = loss;
    rst[RST_ENT] = D.ent;
    rst[RST_LP_MEAN] = (float)lpm;
    rst[RST_LP_STD] = lps;
    rst[RST_LP_MAX] = r.mx; rst[RST_LP_MIN] = r.mn;
  }
}

// ---- the two losses for CategoricalDisPolicy (policies/discrete_policies.py:160-172: log_prob and entropy of
// Categorical(softmax(logits))), in a2c_loss_kernel's / reinforce_loss_kernel's launch position with their records, UpdCtl handling
// and block reductions. p.mean: the logits rows [n][OUT_LD], p.A = K, p.acts: [slots][1] action indices as floats; p.logstd,
// p.dlogstd, p.tanh_action unused. Per row, with p = softmax(z), H its entropy and an the normalised advantage:
//   policy_loss = mean_i(-log p_i[a_i] an_i) - ent_coef mean_i(H_i)
//   d z_j = (1 / n) (-an ([j == a] - p_j) + ent_coef p_j (log p_j + H))       (dH / dz_j = -p_j (log p_j + H))
// written into the d(out) row scaled and clamped like the Gaussian kernels' (grad_out), columns K .. 15 exactly zero.
struct CatLossRow { float lp, ent, an; };
__device__ __forceinline__ CatLossRow cat_loss_row(const ActorArgs& p, int i, float amean, float astd, int& sat) {
  const int K = p.A;
  const int slot = p.rowidx ? p.rowidx[i] : i;
  CatLossRow o;
  o.an = (p.adv[slot] - amean) / (astd + 1e-5f);
  const float act = p.acts[slot];
  const CatDist d = cat_dist(p.mean + (int64_t)i * OUT_LD, K);
  o.lp = cat_logp(d, K, act);
  o.ent = d.ent;
  float dz[CAT_CAP];
#pragma unroll
  for (int j = 0; j < CAT_CAP; ++j) {
    dz[j] = 0.f;
    if (j < K) {
      const float hit = act == (float)j ? 1.f : 0.f;
      dz[j] = grad_out(p.inv_n * (-o.an * (hit - d.p[j]) + p.ent_coef * d.p[j] * (d.lg[j] + d.ent)), p.gscale, sat);
    }
  }
  actor_store_dmean(p.dmean + (int64_t)i * OUT_LD, dz, true);
  return o;
}
// A2C.update's policy loss (a2c.py:61-74) for a categorical policy: fills AST_PI_LOSS, AST_ENT (ent.mean()) and AST_LOGP; the
// record's std/* slots (a2c.py:97-102 logs them only `if 'std' in out`) stay as the caller cleared them.
__global__ __launch_bounds__(1024) void a2c_cat_loss_kernel(ActorArgs p, const UpdCtl* __restrict__ ctl, float* __restrict__ ast_all) {
  const int n = p.n;
  const float amean = p.st[ST_ADV_MEAN], astd = p.st[ST_ADV_STD];
  double s_lp = 0.0, s_loss = 0.0, s_ent = 0.0;
  int sat = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const CatLossRow o = cat_loss_row(p, i, amean, astd, sat);
    s_loss += (double)(-o.lp * o.an);
    s_lp += o.lp;
    s_ent += o.ent;
  }
  const Red4 r = block_red4(s_loss, s_lp, 0.f, 0.f);
  const Red4 r2 = block_red4((double)sat, s_ent, 0.f, 0.f);
  if (threadIdx.x == 0) {
    float* st = p.st;
    const double lpm = r.s2 / n, entm = r2.s2 / n;
    const float loss = (float)(r.s / n - (double)p.ent_coef * entm);
    st[ST_PI_LOSS] = loss;
    st[ST_LP_MEAN] = (float)lpm;
    if (p.gscale != 1.f) st[ST_F16_SAT] += (float)r2.s;
    float* ast = ast_all + (int64_t)ctl->upd_index * AST_SIZE;
    ast[AST_PI_LOSS] = loss;
    ast[AST_ENT] = (float)entm;
    ast[AST_LOGP] = (float)lpm;
  }
}
// Reinforce.update's policy loss (reinforce.py:52-61) for a categorical policy: reinforce_loss_kernel's record, ent = ent.mean().
__global__ __launch_bounds__(1024) void reinforce_cat_loss_kernel(ActorArgs p, const UpdCtl* __restrict__ ctl,
                                                                 float* __restrict__ rst_all) {
  const int n = p.n;
  const float amean = p.st[ST_ADV_MEAN], astd = p.st[ST_ADV_STD];
  double s_lp = 0.0, s_lp2 = 0.0, s_loss = 0.0, s_ent = 0.0;
  float lp_mx = -INFINITY, lp_mn = INFINITY;
  int sat = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const CatLossRow o = cat_loss_row(p, i, amean, astd, sat);
    s_loss += (double)(-o.lp * o.an);
    s_lp += o.lp; s_lp2 += (double)o.lp * o.lp;
    lp_mx = fmaxf(lp_mx, o.lp); lp_mn = fminf(lp_mn, o.lp);
    s_ent += o.ent;
  }
  const Red4 r = block_red4(s_lp, s_lp2, lp_mx, lp_mn);
  const Red4 r2 = block_red4(s_loss, (double)sat, 0.f, 0.f);
  const Red4 r3 = block_red4(s_ent, 0.0, 0.f, 0.f);
  if (threadIdx.x == 0) {
    float* st = p.st;
    const double dn = (double)n;
    const double lpm = r.s / dn, entm = r3.s / dn;
    const float loss = (float)(r2.s / dn - (double)p.ent_coef * entm);
    const float lps = (float)sqrt(fmax(0.0, (r.s2 - dn * lpm * lpm) / (dn - 1.0)));  // (n >= 2: never one element)
    st[ST_PI_LOSS] = loss;
    st[ST_LP_MEAN] = (float)lpm;
    st[ST_LP_STD] = lps;
    st[ST_LP_MAX] = r.mx; st[ST_LP_MIN] = r.mn;
    if (p.gscale != 1.f) st[ST_F16_SAT] += (float)r2.s2;
    float* rst = rst_all + (int64_t)ctl->upd_index * RST_SIZE;
    // advs/std: numpy's (population) std of the host batch, as in reinforce_loss_kernel
    rst[RST_ADV_MEAN] = st[ST_ADV_MEAN]; rst[RST_ADV_STD] = (float)sqrt((double)st[ST_ADV_M2] / dn);
    rst[RST_ADV_MAX] = st[ST_ADV_MAX]; rst[RST_ADV_MIN] = st[ST_ADV_MIN];
    rst[RST_PI_LOSS] = loss;
    rst[RST_ENT] = (float)entm;
    rst[RST_LP_MEAN] = (float)lpm;
    rst[RST_LP_STD] = lps;
    rst[RST_LP_MAX] = r.mx; rst[RST_LP_MIN] = r.mn;
  }
}
#pragma clang fp contract(fast)

// --------------------------------------------------------------------------------- weight packing
// Builds the contraction-ready copies of a weight tensor (operand type T, zero padded to the GEMM tiles).
enum { PK_NT = 0, PK_T = 1, PK_CONV_NHWC = 2, PK_CONV_NHWC_T = 3, PK_CONV_DGRAD = 4, PK_FRAG = 5, PK_FRAGP = 6, PK_FRAGPT = 7, PK_FRAGT = 8 };
struct PackDesc {
  const float* src;  // PyTorch-layout weight
  int64_t dst_off;   // element offset in the packed buffer
  int kind;
  int R, Cc;         // packed rows / cols (padded)
  int N, K;          // source: [N][K] (Linear) or [N][Cin*taps] (Conv)
  int Cin, taps, KW; // conv
  int s, py, px, TW; // dgrad class
  int64_t blk0;
};
// 8 consecutive packed elements (one row: every packed row length is a multiple of 8) per thread, one 16 / 32-byte store
constexpr int PACK_PER_BLOCK = 256 * 8;
template <typename T>
__device__ __forceinline__ void pack_body(const PackDesc* __restrict__ descs, int nd, T* __restrict__ dst, int64_t blk) {
  const PackDesc d = descs[find_desc(descs, nd, blk)];
  const V4L_GLOBAL float* src = as_global(d.src);
  const int64_t e0 = ((blk - d.blk0) * 256 + threadIdx.x) * 8;
  if (e0 >= (int64_t)d.R * d.Cc) return;
  const int r = (int)(e0 / d.Cc), c0 = (int)(e0 - (int64_t)r * d.Cc);
  float val[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int c = c0 + q;
    const int64_t e = e0 + q;
    float v = 0.f;
    switch (d.kind) {
      case PK_FRAG: {  // MFMA fragment order [column tile n/16][k-step k/32][lane = (k%32)/8*16 + n%16][k%8]: the 64 lanes
        // of a wave read one fragment as ONE contiguous 64 x sizeof(fragment) block (8 whole cache lines for bf16)
        const int j = (int)(e & 7), lane = (int)((e >> 3) & 63), blk = (int)(e >> 9), ksteps = d.Cc >> 5;
        const int tile = blk / ksteps, ks = blk - tile * ksteps;
        const int n = tile * 16 + (lane & 15), k = ks * 32 + (lane >> 4) * 8 + j;
        if (n < d.N && k < d.K) {
          if (d.Cin > 0) { const int tap = k / d.Cin, ci = k - tap * d.Cin; v = src[(int64_t)n * d.K + ci * d.taps + tap]; }  // NHWC k order
          else v = src[(int64_t)n * d.K + k];
        }
      } break;
      case PK_FRAGT: {  // PK_FRAG of the TRANSPOSED weight (data-grad GEMMs): rows = input features (NHWC order when
        // d.Cin > 0, like PK_CONV_NHWC_T), contraction index = output feature
        const int j = (int)(e & 7), lane = (int)((e >> 3) & 63), blk = (int)(e >> 9), ksteps = d.Cc >> 5;
        const int tile = blk / ksteps, ks = blk - tile * ksteps;
        const int row = tile * 16 + (lane & 15), k = ks * 32 + (lane >> 4) * 8 + j;
        if (row < d.K && k < d.N) {
          if (d.Cin > 0) { const int tap = row / d.Cin, ci = row - tap * d.Cin; v = src[(int64_t)k * d.K + ci * d.taps + tap]; }
          else v = src[(int64_t)k * d.K + row];
        }
      } break;
      case PK_FRAGP:     // fragment order with the wave-per-sample kernels' k permutation (csrc/wps.h): slot (g = lane >> 4, j)
      case PK_FRAGPT: {  // holds k = 32 ks + 16 (j >> 2) + 4 g + (j & 3). FRAGP: rows = output features n, k = input feature
        // (forward GEMMs); FRAGPT: rows = input features, k = output feature (data-grad GEMMs: the transposed weight)
        const int j = (int)(e & 7), lane = (int)((e >> 3) & 63), blk = (int)(e >> 9), ksteps = d.Cc >> 5;
        const int tile = blk / ksteps, ks = blk - tile * ksteps;
        const int row = tile * 16 + (lane & 15), k = ks * 32 + 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3);
        if (d.kind == PK_FRAGP) { if (row < d.N && k < d.K) v = src[(int64_t)row * d.K + k]; }
        else if (row < d.K && k < d.N) v = src[(int64_t)k * d.K + row];
      } break;
      // (d.px: the source's K axis starts at packed column / row px — the vision-only Transformer's first head layer inside
      // the 128-wide pooled operand of the wave-per-sample kernels, csrc/wps.h; 0 everywhere else)
      case PK_NT: if (r < d.N && c >= d.px && c - d.px < d.K) v = src[(int64_t)r * d.K + (c - d.px)]; break;
      case PK_T: if (r >= d.px && r - d.px < d.K && c < d.N) v = src[(int64_t)c * d.K + (r - d.px)]; break;
      case PK_CONV_NHWC:  // dst[n][tap*Cin+ci] = W[n][ci][tap]
        if (r < d.N && c < d.K) { const int tap = c / d.Cin, ci = c - tap * d.Cin; v = src[(int64_t)r * d.K + ci * d.taps + tap]; }
        break;
      case PK_CONV_NHWC_T:  // dst[tap*Cin+ci][n] = W[n][ci][tap]
        if (r < d.K && c < d.N) { const int tap = r / d.Cin, ci = r - tap * d.Cin; v = src[(int64_t)c * d.K + ci * d.taps + tap]; }
        break;
      case PK_CONV_DGRAD: {  // dst[ci][(a*TW+bb)*N + n] = W[n][ci][py+s*a][px+s*bb]
        const int kk = d.TW * d.TW * d.N;
        if (r < d.Cin && c < kk) {
          const int tap = c / d.N, n = c - tap * d.N;
          const int a = tap / d.TW, bb = tap - a * d.TW;
          const int ky = d.py + d.s * a, kx = d.px + d.s * bb;
          v = src[(int64_t)n * d.K + r * d.taps + ky * d.KW + kx];
        }
      } break;
    }
    val[q] = v;
  }
  T* o = dst + d.dst_off + e0;
  st4(o, val[0], val[1], val[2], val[3]);
  st4(o + 4, val[4], val[5], val[6], val[7]);
}
template <typename T>
__global__ __launch_bounds__(256) void pack_kernel(const PackDesc* __restrict__ descs, int nd, T* __restrict__ dst) {
  pack_body<T>(descs, nd, dst, (int64_t)blockIdx.x);
}
// The first launch of an update: block 0 opens the update (upd_begin_body), the others refresh the critic's operand-type
// weight copies — two independent latency chains that used to be two launches back to back.
template <typename T>
__global__ __launch_bounds__(256) void begin_pack_kernel(UpdCtl* c, const int* __restrict__ rowidx_all, int n, int* rowidx_cur,
                                                         float* stats_cur, const float* __restrict__ adv,
                                                         const PackDesc* __restrict__ descs, int nd, T* __restrict__ dst) {
  if (blockIdx.x == 0) upd_begin_body(c, rowidx_all, n, rowidx_cur, stats_cur, adv);
  else pack_body<T>(descs, nd, dst, (int64_t)blockIdx.x - 1);
}

// --------------------------------------------------------------------------------- GAE
// torchrl/replay_buffers/on_policy.py:17-45 — fp64, same expression order as the numpy code, FMA contraction
// off, so the result is bit-identical to the reference's (then optionally cast once to fp32, as ppo.py:138,140
// does). Two phases: (1) everything that does not depend on the recursion — delta_t, the carry coefficient
// ((1-term)*gamma)*tau and the time-limit factor — is computed fully parallel over [T,E]; (2) the 3-flop
// recursion runs one lane per env over t with the loads of 8 steps in flight (they do not depend on A).
// tl_stride_e: 0 when _time_limits is [T,1] (broadcast over envs), 1 when [T,E,1].
__global__ __launch_bounds__(256) void gae_prep_kernel(const double* __restrict__ rewards, const double* __restrict__ values,
                                                       const double* __restrict__ terminals,
                                                       const double* __restrict__ time_limits, int tl_stride_e,
                                                       const double* __restrict__ last_value, int T, int E, double gamma,
                                                       double tau, int use_tl, double* __restrict__ delta,
                                                       double* __restrict__ coef, double* __restrict__ tlm) {
#pragma clang fp contract(off)
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= (int64_t)T * E) return;
  const int t = (int)(o / E), e = (int)(o - (int64_t)t * E);
  const double c = (1.0 - terminals[o]) * gamma;
  const double vnext = (t == T - 1) ? last_value[e] : values[o + E];
  double d = rewards[o] + c * vnext;
  d = d - values[o];
  delta[o] = d;
  coef[o] = c * tau;
  tlm[o] = use_tl ? (1.0 - time_limits[tl_stride_e ? o : t]) : 1.0;
}

__global__ void gae_scan_kernel(const double* __restrict__ delta, const double* __restrict__ coef,
                                const double* __restrict__ tlm, const double* __restrict__ values, int T, int E,
                                int use_tl, double* __restrict__ advs, double* __restrict__ rets,
                                float* __restrict__ advs32, float* __restrict__ rets32) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  double A = 0.0;
  for (int t0 = T - 1; t0 >= 0; t0 -= 8) {
    double d[8], c[8], m[8], v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int t = t0 - j;
      const int64_t o = (int64_t)(t < 0 ? 0 : t) * E + e;
      d[j] = delta[o]; c[j] = coef[o]; m[j] = tlm[o]; v[j] = values[o];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int t = t0 - j;
      if (t < 0) break;
      const int64_t o = (int64_t)t * E + e;
      A = d[j] + c[j] * A;
      if (use_tl) A = A * m[j];
      const double r = A + v[j];
      advs[o] = A;
      rets[o] = r;
      if (advs32 != nullptr) { advs32[o] = (float)A; rets32[o] = (float)r; }
    }
  }
}

// discount_reward (PPO(gae=False)): torchrl/replay_buffers/on_policy.py:47-71 — fp64, the numpy expression order, FMA
// contraction off: bit-identical to the reference. One lane per env walks t = T-1 .. 0 with 8 steps' loads in flight.
//   time-limit filter:  R = (r + (((1 - term) * gamma) * R) * (1 - tl)) + tl * V;   else:  R = r + ((1 - term) * gamma) * R
//   advs = R - V, estimate_returns = R.
__global__ void discount_scan_kernel(const double* __restrict__ rewards, const double* __restrict__ values,
                                     const double* __restrict__ terminals, const double* __restrict__ time_limits,
                                     int tl_stride_e, const double* __restrict__ last_value, int T, int E, double gamma,
                                     int use_tl, double* __restrict__ advs, double* __restrict__ rets,
                                     float* __restrict__ advs32, float* __restrict__ rets32) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  double R = last_value[e];
  for (int t0 = T - 1; t0 >= 0; t0 -= 8) {
    double r[8], c[8], m[8], v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int t = t0 - j < 0 ? 0 : t0 - j;
      const int64_t o = (int64_t)t * E + e;
      r[j] = rewards[o]; v[j] = values[o];
      c[j] = (1.0 - terminals[o]) * gamma;
      m[j] = use_tl ? time_limits[tl_stride_e ? o : t] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int t = t0 - j;
      if (t < 0) break;
      const int64_t o = (int64_t)t * E + e;
      double x = c[j] * R;
      if (use_tl) {
        x = x * (1.0 - m[j]);
        x = r[j] + x;
        R = x + m[j] * v[j];
      } else {
        R = r[j] + x;
      }
      const double a = R - v[j];
      advs[o] = a;
      rets[o] = R;
      if (advs32 != nullptr) { advs32[o] = (float)a; rets32[o] = (float)R; }
    }
  }
}

// Running observation normaliser of the vectorised env: NormObsWithImg.observation (vision4leg/get_env.py:58-67) /
// NormObs.observation (torchrl/env/base_wrapper.py:119-122) on the [E][S] proprio block of one env step —
// Normalizer.update_estimate (base_wrapper.py:77-84: merge the batch mean / variance over the E envs into the running
// statistics with update_mean_var_count, :44-61) when `update`, then Normalizer.filt (:93-96) with the new statistics.
// fp64, the numpy expression order (axis-0 reductions run row after row), FMA contraction off: bit-identical to the
// reference; out32 is the fp32 cast the collector's torch.Tensor(ob) makes (collector/on_policy.py:93). Block 0 owns
// the statistics (one lane per proprio dimension: its E raw values are one coalesced column walk, nothing is shared
// between lanes but the count); blocks 1.. move the step's depth stack into the same fp32 observation rows (the
// reference's per-step np.hstack of a 16 K-float image row), converting from fp64 when the env hands that over.
struct ObsNorm {
  const double* raw; int64_t ld_raw;       // [E][S] raw proprio rows
  double *mean, *var, *count;              // [S], [S], [1] running statistics (updated in place)
  double clip; int E, S, update;
  float* out32; int64_t ld32;              // normalised rows as fp32 (nullable)
  double* out64; int64_t ld64;             // ... and as fp64 (nullable)
  const void* img; int img_f64; int64_t ld_img, img_elems;  // [E][img_elems] fp32 / fp64 depth stack (nullable)
  float* img_out; int64_t ld_img_out;
};

__global__ __launch_bounds__(256) void obs_norm_kernel(ObsNorm p) {
#pragma clang fp contract(off)
  if (blockIdx.x != 0) {
    const int64_t n = (int64_t)p.E * p.img_elems, step = (int64_t)(gridDim.x - 1) * 256;
    for (int64_t i = (int64_t)(blockIdx.x - 1) * 256 + threadIdx.x; i < n; i += step) {
      const int64_t e = i / p.img_elems, c = i - e * p.img_elems;
      const float v = p.img_f64 ? (float)((const double*)p.img)[e * p.ld_img + c] : ((const float*)p.img)[e * p.ld_img + c];
      p.img_out[e * p.ld_img_out + c] = v;
    }
    return;
  }
  const double cnt = *p.count, bc = (double)p.E;
  __syncthreads();  // every lane holds the old count before lane 0 replaces it
  for (int d = threadIdx.x; d < p.S; d += 256) {
    const double* col = p.raw + d;
    double m = p.mean[d], v = p.var[d];
    // the column's E values, 8 loads in flight at a time (the adds below are sequential by contract, the loads are not)
    auto walk = [&](auto&& f) {
      for (int e0 = 0; e0 < p.E; e0 += 8) {
        double c[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) c[j] = col[(int64_t)(e0 + j < p.E ? e0 + j : e0) * p.ld_raw];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (e0 + j < p.E) f(e0 + j, c[j]);
      }
    };
    if (p.update) {
      double s = 0.0;
      walk([&](int e, double c) { s = e == 0 ? c : s + c; });
      const double bm = s / bc;
      double q = 0.0;
      walk([&](int e, double c) {
        const double x = c - bm;
        q = e == 0 ? x * x : q + x * x;
      });
      const double bv = q / bc;
      const double delta = bm - m, tot = cnt + bc;
      const double new_mean = m + delta * bc / tot;
      const double m_a = v * cnt, m_b = bv * bc;
      const double M2 = m_a + m_b + delta * delta * cnt * bc / tot;
      m = new_mean;
      v = M2 / tot;
      p.mean[d] = m;
      p.var[d] = v;
    }
    const double den = sqrt(v) + 1e-4;
    walk([&](int e, double c) {
      double y = (c - m) / den;
      y = y < -p.clip ? -p.clip : y;
      y = y > p.clip ? p.clip : y;
      if (p.out64 != nullptr) p.out64[e * p.ld64 + d] = y;
      if (p.out32 != nullptr) p.out32[e * p.ld32 + d] = (float)y;
    });
  }
  if (p.update && threadIdx.x == 0) *p.count = cnt + bc;
}

}  // namespace v4l
