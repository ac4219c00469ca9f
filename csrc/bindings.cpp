// pertgnn._C — Python bindings for the CDNA4 kernel library.
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <climits>
#include <cstdlib>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include <c10/cuda/CUDAStream.h>

#include "hip/gemm_dispatch.h"
#include "hip/launchers.h"

namespace {

#define CHECK_IN(t)                                                      \
  TORCH_CHECK((t).is_cuda(), #t " must be on GPU");                      \
  TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")

inline hipStream_t cur_stream() {
  return (hipStream_t)c10::cuda::getCurrentCUDAStream().stream();
}

using OptTensor = std::optional<torch::Tensor>;

// A gradient sink is the optimizer's fp32 flat-gradient slice of a parameter,
// handed to a backward op as the destination of that parameter's gradient:
// the op ADDS into it (plain read-modify-write where one thread owns the
// element, atomicAdd where several combine) and never clears or stores, so
// the result is what autograd's accumulation of a returned gradient would
// have left there.  A sink is only 4-byte aligned (flat offsets are sums of
// numel()) and sits between other parameters' gradients: the epilogues that
// write one are scalar.  -> its pointer, or nullptr if there is none; a sink
// of the wrong kind is an error, never a silent fall-back.
inline float* grad_sink(const OptTensor& sink, const torch::Tensor& like,
                        at::IntArrayRef shape, const char* what) {
  if (!sink.has_value() || !sink->defined()) return nullptr;
  TORCH_CHECK(sink->is_cuda() && sink->device() == like.device(), what,
              ": the gradient sink must be on the op's GPU");
  TORCH_CHECK(sink->scalar_type() == torch::kFloat32, what,
              ": the gradient sink must be float32");
  TORCH_CHECK(sink->is_contiguous(), what,
              ": the gradient sink must be contiguous");
  TORCH_CHECK(sink->sizes() == shape, what, ": the gradient sink must be ",
              shape, ", got ", sink->sizes());
  return sink->data_ptr<float>();
}

// dgamma/dbeta of a BN backward: both sinks or neither
struct BnAffineOut {
  torch::Tensor dgamma, dbeta;  // what the op returns ([0] when sunk)
  float* pg;
  float* pb;
  bool acc;
};
inline BnAffineOut bn_affine_out(const OptTensor& dgamma_sink,
                                 const OptTensor& dbeta_sink,
                                 const torch::Tensor& like, int h,
                                 const char* what) {
  BnAffineOut o;
  o.pg = grad_sink(dgamma_sink, like, {h}, what);
  o.pb = grad_sink(dbeta_sink, like, {h}, what);
  TORCH_CHECK((o.pg != nullptr) == (o.pb != nullptr), what,
              ": dgamma and dbeta sinks come together");
  o.acc = o.pg != nullptr;
  auto fopt = like.options().dtype(torch::kFloat32);
  o.dgamma = torch::empty({o.acc ? 0 : h}, fopt);
  o.dbeta = torch::empty({o.acc ? 0 : h}, fopt);
  if (!o.acc) {
    o.pg = o.dgamma.data_ptr<float>();
    o.pb = o.dbeta.data_ptr<float>();
  }
  return o;
}

}  // namespace

// csrc/collate.cpp
std::vector<torch::Tensor> collate_native(
    std::vector<torch::Tensor>, std::vector<torch::Tensor>,
    std::vector<torch::Tensor>, std::vector<torch::Tensor>,
    std::vector<torch::Tensor>, std::vector<torch::Tensor>,
    std::vector<torch::Tensor>, std::vector<torch::Tensor>,
    std::vector<torch::Tensor>, bool);

// ---------------------------------------------------------------------------

std::vector<torch::Tensor> edge_attn_fwd(torch::Tensor q, torch::Tensor k,
                                         torch::Tensor v, torch::Tensor e,
                                         torch::Tensor row_ptr,
                                         torch::Tensor csr_src,
                                         torch::Tensor skip) {
  CHECK_IN(q); CHECK_IN(k); CHECK_IN(v); CHECK_IN(e);
  CHECK_IN(row_ptr); CHECK_IN(csr_src);
  const int n = q.size(0);
  const int h = q.size(1);
  TORCH_CHECK(h <= 512, "H must be <= 512");
  auto out = torch::empty_like(q);
  auto alpha = torch::empty({e.size(0)}, q.options());
  const float* skip_p = nullptr;
  if (skip.defined() && skip.numel() > 0) {
    CHECK_IN(skip);
    skip_p = skip.data_ptr<float>();
  }
  launch_edge_attn_fwd(q.data_ptr<float>(), k.data_ptr<float>(),
                       v.data_ptr<float>(), e.data_ptr<float>(),
                       row_ptr.data_ptr<int>(), csr_src.data_ptr<int>(),
                       skip_p, out.data_ptr<float>(), alpha.data_ptr<float>(),
                       n, h, cur_stream());
  return {out, alpha};
}

std::vector<torch::Tensor> edge_attn_bwd(
    torch::Tensor g, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor e, torch::Tensor alpha, torch::Tensor row_ptr,
    torch::Tensor csr_src, torch::Tensor col_ptr, torch::Tensor csc_dst,
    torch::Tensor csc_eid) {
  CHECK_IN(g); CHECK_IN(q); CHECK_IN(alpha);
  const int n = q.size(0);
  const int h = q.size(1);
  const long ne = e.size(0);
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);
  auto de = torch::empty_like(e);
  auto dek = torch::empty_like(e);
  auto dev = torch::empty_like(e);
  launch_edge_attn_bwd(g.data_ptr<float>(), q.data_ptr<float>(),
                       k.data_ptr<float>(), v.data_ptr<float>(),
                       e.data_ptr<float>(), alpha.data_ptr<float>(),
                       row_ptr.data_ptr<int>(), csr_src.data_ptr<int>(),
                       col_ptr.data_ptr<int>(), csc_eid.data_ptr<int>(),
                       dq.data_ptr<float>(), dk.data_ptr<float>(),
                       dv.data_ptr<float>(), de.data_ptr<float>(),
                       dek.data_ptr<float>(), dev.data_ptr<float>(), n, h, ne,
                       cur_stream());
  return {dq, dk, dv, de};
}

// partial sums per graph of the pattern pool's first pass: about 8192 over
// the batch, no more than a graph's share of the n rows, 1..64
static long seg_pool_parts(long n, int64_t num_graphs) {
  const long graphs = std::max<int64_t>(num_graphs, 1);
  const long per_g = (n + graphs - 1) / graphs;
  return std::min<long>(std::max<long>(std::min(8192 / graphs, per_g), 1), 64);
}

torch::Tensor seg_pool_fwd(torch::Tensor x, torch::Tensor probs,
                           torch::Tensor nn, torch::Tensor batch_ptr,
                           int64_t num_graphs) {
  CHECK_IN(x); CHECK_IN(probs); CHECK_IN(nn); CHECK_IN(batch_ptr);
  const int h = x.size(1);
  const long p = seg_pool_parts(x.size(0), num_graphs);
  auto partial = torch::empty({num_graphs * p, h}, x.options());
  auto out = torch::empty({num_graphs, h}, x.options());
  launch_seg_pool_fwd(x.data_ptr<float>(), probs.data_ptr<float>(),
                      nn.data_ptr<float>(), batch_ptr.data_ptr<int>(),
                      partial.data_ptr<float>(), out.data_ptr<float>(),
                      (int)num_graphs, (int)p, h, cur_stream());
  return out;
}

torch::Tensor seg_pool_bwd(torch::Tensor gout, torch::Tensor probs,
                           torch::Tensor nn, torch::Tensor batch) {
  CHECK_IN(gout); CHECK_IN(batch);
  const long n = batch.size(0);
  const int h = gout.size(1);
  auto dx = torch::empty({n, h}, gout.options());
  launch_seg_pool_bwd(gout.data_ptr<float>(), probs.data_ptr<float>(),
                      nn.data_ptr<float>(), batch.data_ptr<long>(),
                      dx.data_ptr<float>(), n, h, cur_stream());
  return dx;
}

torch::Tensor embed_node_fwd(torch::Tensor x_raw, torch::Tensor idx,
                             torch::Tensor table, bool out16 = false,
                             int64_t pad_to = 0) {
  CHECK_IN(x_raw); CHECK_IN(idx); CHECK_IN(table);
  const long n = x_raw.size(0);
  const int f = x_raw.size(1);
  const int h = table.size(1);
  if (pad_to != 0) {
    // [n, pad_to]: the concat in the first f + h columns, +0 in the rest
    TORCH_CHECK(pad_to >= f + h && pad_to <= INT_MAX,
                "embed_node_fwd: pad_to=", pad_to, " is below f + h = ", f + h);
    auto out = torch::empty(
        {n, pad_to}, out16 ? x_raw.options().dtype(torch::kBFloat16)
                           : x_raw.options());
    launch_embed_node_pad(x_raw.data_ptr<float>(), idx.data_ptr<long>(),
                          table.data_ptr<float>(), out.data_ptr(),
                          out16 ? 1 : 0, n, f, h, (int)pad_to, cur_stream());
    return out;
  }
  if (out16) {
    auto out = torch::empty({n, f + h},
                            x_raw.options().dtype(torch::kBFloat16));
    launch_embed_node_fwd16(x_raw.data_ptr<float>(), idx.data_ptr<long>(),
                            table.data_ptr<float>(), out.data_ptr(), n, f, h,
                            cur_stream());
    return out;
  }
  auto out = torch::empty({n, f + h}, x_raw.options());
  launch_embed_node_fwd(x_raw.data_ptr<float>(), idx.data_ptr<long>(),
                        table.data_ptr<float>(), out.data_ptr<float>(), n, f,
                        h, cur_stream());
  return out;
}

torch::Tensor embed_edge_fwd(torch::Tensor attr, torch::Tensor ifc,
                             torch::Tensor rpc) {
  CHECK_IN(attr); CHECK_IN(ifc); CHECK_IN(rpc);
  const long e = attr.size(0);
  const int h = ifc.size(1);
  const int astride = attr.size(1);
  auto out = torch::empty({e, 2 * h}, ifc.options());
  launch_embed_edge_fwd(attr.data_ptr<long>(), ifc.data_ptr<float>(),
                        rpc.data_ptr<float>(), out.data_ptr<float>(), e, h,
                        astride, cur_stream());
  return out;
}

torch::Tensor gather_rows(torch::Tensor idx, torch::Tensor table) {
  CHECK_IN(idx); CHECK_IN(table);
  const long n = idx.size(0);
  const int h = table.size(1);
  auto out = torch::empty({n, h}, table.options());
  launch_gather_rows(idx.data_ptr<long>(), table.data_ptr<float>(),
                     out.data_ptr<float>(), n, h, cur_stream());
  return out;
}

static const unsigned long long* rng_seed_ptr(torch::Tensor& seed,
                                              double dropout_p) {
  if (dropout_p <= 0.0 || !seed.defined() || seed.numel() == 0) return nullptr;
  TORCH_CHECK(seed.scalar_type() == torch::kLong && seed.is_cuda(),
              "dropout seed must be an int64 CUDA scalar");
  return (const unsigned long long*)seed.data_ptr<long>();
}

// Per-call slab of the wide BN reductions (one [2h] row per block, folded in
// fixed order).  Caching-allocator memory is stream-ordered, so this is safe
// under hipGraph capture and when BN calls overlap on a side stream.
static torch::Tensor bn_wide_slab(const torch::Tensor& x) {
  const long rows = bn_wide_slab_rows(x.size(0), (int)x.size(1));
  return torch::empty({rows, 2 * x.size(1)},
                      x.options().dtype(torch::kFloat32));
}
static float* bn_slab_ptr(const torch::Tensor& slab) {
  return slab.numel() ? slab.data_ptr<float>() : nullptr;
}
// y-or-mask argument of the act16 backward entry points: a uint8 tensor is
// the bit-packed keep mask [n, h/8] of the forward, anything else is y
static const unsigned char* bn_mask_ptr(const torch::Tensor& ym,
                                        const torch::Tensor& x) {
  if (ym.scalar_type() != torch::kUInt8) return nullptr;
  TORCH_CHECK(ym.is_contiguous() && x.size(1) % 8 == 0 &&
                  ym.numel() == x.size(0) * (x.size(1) / 8) &&
                  bn_wide_ok((int)x.size(1)),
              "BN keep mask must be a contiguous uint8 [n, h/8] tensor");
  return ym.data_ptr<unsigned char>();
}
// keep mask written by a training forward with ReLU on a fast-path shape
// (empty tensor otherwise: eval mode, relu=false and other shapes write none)
static torch::Tensor bn_new_mask(const torch::Tensor& x, bool training,
                                 bool relu) {
  const long n = x.size(0), h = x.size(1);
  const bool on = training && relu && n > 0 && bn_wide_ok((int)h);
  return torch::empty({on ? n : 0, on ? h / 8 : 0},
                      x.options().dtype(torch::kUInt8));
}

// ---------------------------------------------------------------------------
// BatchNorm(+ReLU+dropout).  Every operation is one function for both
// activation dtypes, dispatching on x.scalar_type(): fp32, or bf16 (act16:
// the x, y, g and dx streams are bf16; statistics, affine parameters and
// their gradients stay fp32).  It is bound under two Python names that are
// aliases checking the dtype: the plain one (A16 = false) requires fp32
// activations, the "16" one bf16.  The bf16 forwards also return the keep
// mask (empty where none is written), so they return four tensors, the fp32
// ones three.
// ---------------------------------------------------------------------------

// The gate of the BN bindings: x is [n, h] of the dtype the name requires; g
// (a backward's incoming gradient) matches it in dtype and shape; ym is y,
// or for bf16 the uint8 keep mask that bn_mask_ptr accepts.  -> x is bf16
static bool bn_gate(const char* name, bool a16, const torch::Tensor& x,
                    const torch::Tensor* g = nullptr,
                    const torch::Tensor* ym = nullptr) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2, name,
              ": x must be a contiguous [n, h] GPU tensor");
  TORCH_CHECK(x.size(1) <= INT_MAX, name, ": h does not fit an int");
  TORCH_CHECK(x.scalar_type() == (a16 ? torch::kBFloat16 : torch::kFloat32),
              name, " takes ", a16 ? "bf16" : "fp32", " activations, got ",
              x.scalar_type(), a16 ? " (fp32 ones go to the name without 16)"
                                   : " (bf16 ones go to the name with 16)");
  if (g)
    TORCH_CHECK(g->is_cuda() && g->is_contiguous() &&
                    g->scalar_type() == x.scalar_type() &&
                    g->sizes() == x.sizes(),
                name, ": g must match x in dtype and shape, got ",
                g->scalar_type(), " ", g->sizes(), " for x ", x.sizes());
  if (ym && !(a16 && ym->scalar_type() == torch::kUInt8))
    TORCH_CHECK(ym->is_cuda() && ym->is_contiguous() &&
                    ym->scalar_type() == x.scalar_type() &&
                    ym->sizes() == x.sizes(),
                name, ": y must match x in dtype and shape",
                a16 ? " (or be the uint8 keep mask)" : "");
  return x.scalar_type() == torch::kBFloat16;
}

static void bn_partials_check(const char* name, const torch::Tensor& partials,
                              int h) {
  TORCH_CHECK(partials.numel() == 2 * h + 1, name,
              " expects [2h+1] partials with the global count in the tail "
              "slot");
}

template <bool A16>
std::vector<torch::Tensor> bn_relu_fwd(torch::Tensor x, torch::Tensor gamma,
                                       torch::Tensor beta,
                                       torch::Tensor running_mean,
                                       torch::Tensor running_var,
                                       double momentum, double eps,
                                       bool training, bool relu,
                                       double dropout_p, torch::Tensor seed) {
  const bool b16 = bn_gate(A16 ? "bn_relu_fwd16" : "bn_relu_fwd", A16, x);
  CHECK_IN(gamma); CHECK_IN(beta);
  const long n = x.size(0);
  const int h = x.size(1);
  auto fopt = x.options().dtype(torch::kFloat32);
  auto y = torch::empty_like(x);
  auto mean = torch::empty({h}, fopt);
  auto invstd = torch::empty({h}, fopt);
  auto partials = torch::empty({2 * h}, fopt);
  auto slab = training ? bn_wide_slab(x) : torch::empty({0}, fopt);
  const auto* sp = rng_seed_ptr(seed, dropout_p);
  torch::Tensor mask;
  if (b16) {
    mask = bn_new_mask(x, training, relu);
    launch_bn_fwd16(x.data_ptr(), gamma.data_ptr<float>(),
                    beta.data_ptr<float>(), running_mean.data_ptr<float>(),
                    running_var.data_ptr<float>(), mean.data_ptr<float>(),
                    invstd.data_ptr<float>(), partials.data_ptr<float>(),
                    y.data_ptr(), n, h, (float)momentum, (float)eps, training,
                    relu, (float)dropout_p, sp, bn_slab_ptr(slab),
                    mask.numel() ? mask.data_ptr<unsigned char>() : nullptr,
                    cur_stream());
  } else {
    launch_bn_fwd(x.data_ptr<float>(), gamma.data_ptr<float>(),
                  beta.data_ptr<float>(), running_mean.data_ptr<float>(),
                  running_var.data_ptr<float>(), mean.data_ptr<float>(),
                  invstd.data_ptr<float>(), partials.data_ptr<float>(),
                  y.data_ptr<float>(), n, h, (float)momentum, (float)eps,
                  training, relu, (float)dropout_p, sp, bn_slab_ptr(slab),
                  cur_stream());
  }
  if (sp) launch_counter_bump((unsigned long long*)seed.data_ptr<long>(),
                              cur_stream());
  if (b16) return {y, mean, invstd, mask};
  return {y, mean, invstd};
}

template <bool A16>
std::vector<torch::Tensor> bn_relu_bwd(torch::Tensor g, torch::Tensor x,
                                       torch::Tensor gamma, torch::Tensor mean,
                                       torch::Tensor invstd, torch::Tensor y,
                                       bool relu, double keep_inv,
                                       OptTensor dgamma_sink,
                                       OptTensor dbeta_sink) {
  const char* name = A16 ? "bn_relu_bwd16" : "bn_relu_bwd";
  const bool b16 = bn_gate(name, A16, x, &g, &y);
  const long n = x.size(0);
  const int h = x.size(1);
  auto dx = torch::empty_like(x);
  auto aff = bn_affine_out(dgamma_sink, dbeta_sink, x, h, name);
  auto partials =
      torch::empty({2 * h}, x.options().dtype(torch::kFloat32));
  auto slab = bn_wide_slab(x);
  if (b16)
    launch_bn_bwd16(g.data_ptr(), x.data_ptr(), y.data_ptr(),
                    mean.data_ptr<float>(), invstd.data_ptr<float>(),
                    gamma.data_ptr<float>(), partials.data_ptr<float>(),
                    dx.data_ptr(), aff.pg, aff.pb, n, h, relu, (float)keep_inv,
                    bn_slab_ptr(slab), bn_mask_ptr(y, x), cur_stream(),
                    aff.acc);
  else
    launch_bn_bwd(g.data_ptr<float>(), x.data_ptr<float>(),
                  y.data_ptr<float>(), mean.data_ptr<float>(),
                  invstd.data_ptr<float>(), gamma.data_ptr<float>(),
                  partials.data_ptr<float>(), dx.data_ptr<float>(), aff.pg,
                  aff.pb, n, h, relu, (float)keep_inv, bn_slab_ptr(slab),
                  cur_stream(), aff.acc);
  return {dx, aff.dgamma, aff.dbeta};
}

// The sync-BN pieces.  Partials are [2h+1]: per-channel sum / sum-of-squares
// (backward: of gm and gm*xhat) plus the row count in the tail slot, so a
// single all-reduce carries sums AND the global count with no host
// round-trip (SURVEY.md §7 hard part 4).
template <bool A16>
std::vector<torch::Tensor> bn_finalize_apply(
    torch::Tensor x, torch::Tensor partials, torch::Tensor gamma,
    torch::Tensor beta, torch::Tensor running_mean, torch::Tensor running_var,
    double momentum, double eps, bool training, bool relu, double dropout_p,
    torch::Tensor seed) {
  const char* name = A16 ? "bn_finalize_apply16" : "bn_finalize_apply";
  const bool b16 = bn_gate(name, A16, x);
  CHECK_IN(partials);
  const int h = x.size(1);
  bn_partials_check(name, partials, h);
  auto fopt = x.options().dtype(torch::kFloat32);
  auto y = torch::empty_like(x);
  auto mean = torch::empty({h}, fopt);
  auto invstd = torch::empty({h}, fopt);
  const auto* sp = rng_seed_ptr(seed, dropout_p);
  const float* pp = partials.data_ptr<float>();
  torch::Tensor mask;
  if (b16) {
    mask = bn_new_mask(x, training, relu);
    launch_bn_finalize_apply16(
        x.data_ptr(), pp, pp + 2 * h, gamma.data_ptr<float>(),
        beta.data_ptr<float>(), running_mean.data_ptr<float>(),
        running_var.data_ptr<float>(), mean.data_ptr<float>(),
        invstd.data_ptr<float>(), y.data_ptr(), x.size(0), h, (float)momentum,
        (float)eps, training, relu, (float)dropout_p, sp,
        mask.numel() ? mask.data_ptr<unsigned char>() : nullptr, cur_stream());
  } else {
    launch_bn_finalize_apply(
        x.data_ptr<float>(), pp, pp + 2 * h, gamma.data_ptr<float>(),
        beta.data_ptr<float>(), running_mean.data_ptr<float>(),
        running_var.data_ptr<float>(), mean.data_ptr<float>(),
        invstd.data_ptr<float>(), y.data_ptr<float>(), x.size(0), h,
        (float)momentum, (float)eps, training, relu, (float)dropout_p, sp,
        cur_stream());
  }
  if (sp) launch_counter_bump((unsigned long long*)seed.data_ptr<long>(),
                              cur_stream());
  if (b16) return {y, mean, invstd, mask};
  return {y, mean, invstd};
}

template <bool A16>
torch::Tensor bn_bwd_partials(torch::Tensor g, torch::Tensor x,
                              torch::Tensor y, torch::Tensor mean,
                              torch::Tensor invstd, bool relu,
                              double keep_inv) {
  const bool b16 = bn_gate(A16 ? "bn_bwd_partials16" : "bn_bwd_partials", A16,
                           x, &g, &y);
  const long h = x.size(1);
  auto partials =
      torch::empty({2 * h + 1}, x.options().dtype(torch::kFloat32));
  auto slab = bn_wide_slab(x);
  if (b16)
    launch_bn_bwd_partials_only16(
        g.data_ptr(), x.data_ptr(), y.data_ptr(), mean.data_ptr<float>(),
        invstd.data_ptr<float>(), x.size(0), h, relu,
        partials.data_ptr<float>(), (float)keep_inv, bn_slab_ptr(slab),
        bn_mask_ptr(y, x), cur_stream());
  else
    launch_bn_bwd_partials_only(
        g.data_ptr<float>(), x.data_ptr<float>(), y.data_ptr<float>(),
        mean.data_ptr<float>(), invstd.data_ptr<float>(), x.size(0), h, relu,
        partials.data_ptr<float>(), (float)keep_inv, bn_slab_ptr(slab),
        cur_stream());
  partials.narrow(0, 2 * h, 1).fill_((float)x.size(0));
  return partials;
}

template <bool A16>
std::vector<torch::Tensor> bn_bwd_apply(
    torch::Tensor g, torch::Tensor x, torch::Tensor y, torch::Tensor mean,
    torch::Tensor invstd, torch::Tensor gamma, torch::Tensor partials_global,
    torch::Tensor partials_local, bool relu, double keep_inv,
    OptTensor dgamma_sink, OptTensor dbeta_sink) {
  const char* name = A16 ? "bn_bwd_apply16" : "bn_bwd_apply";
  const bool b16 = bn_gate(name, A16, x, &g, &y);
  const int h = x.size(1);
  bn_partials_check(name, partials_global, h);
  auto dx = torch::empty_like(x);
  auto aff = bn_affine_out(dgamma_sink, dbeta_sink, x, h, name);
  const float* pg = partials_global.data_ptr<float>();
  if (b16)
    launch_bn_bwd_apply_only16(
        g.data_ptr(), x.data_ptr(), y.data_ptr(), mean.data_ptr<float>(),
        invstd.data_ptr<float>(), gamma.data_ptr<float>(), pg, pg + 2 * h,
        dx.data_ptr(), x.size(0), h, relu, (float)keep_inv, bn_mask_ptr(y, x),
        cur_stream());
  else
    launch_bn_bwd_apply_only(
        g.data_ptr<float>(), x.data_ptr<float>(), y.data_ptr<float>(),
        mean.data_ptr<float>(), invstd.data_ptr<float>(),
        gamma.data_ptr<float>(), pg, pg + 2 * h, dx.data_ptr<float>(),
        x.size(0), h, relu, (float)keep_inv, cur_stream());
  launch_bn_grad_affine(partials_local.data_ptr<float>(), aff.pg, aff.pb, h,
                        cur_stream(), aff.acc);
  return {dx, aff.dgamma, aff.dbeta};
}

torch::Tensor quantile_loss_fwd(torch::Tensor y, torch::Tensor y_hat,
                                double tau) {
  CHECK_IN(y); CHECK_IN(y_hat);
  auto out = torch::empty({}, y_hat.options());
  launch_quantile_loss_fwd(y.data_ptr<float>(), y_hat.data_ptr<float>(),
                           out.data_ptr<float>(), y.size(0), (float)tau,
                           cur_stream());
  return out;
}

torch::Tensor quantile_loss_bwd(torch::Tensor g, torch::Tensor y,
                                torch::Tensor y_hat, double tau) {
  auto gc = g.contiguous();
  auto dy_hat = torch::empty_like(y_hat);
  launch_quantile_loss_bwd(gc.data_ptr<float>(), y.data_ptr<float>(),
                           y_hat.data_ptr<float>(), dy_hat.data_ptr<float>(),
                           y.size(0), (float)tau, cur_stream());
  return dy_hat;
}

std::vector<torch::Tensor> eval_metrics(torch::Tensor y, torch::Tensor y_hat,
                                        double tau) {
  CHECK_IN(y); CHECK_IN(y_hat);
  auto out3 = torch::empty({3}, y_hat.options());
  launch_eval_metrics(y.data_ptr<float>(), y_hat.data_ptr<float>(),
                      out3.data_ptr<float>(), y.size(0), (float)tau,
                      cur_stream());
  return {out3[0], out3[1], out3[2]};
}

void adam_step(torch::Tensor p, torch::Tensor g, torch::Tensor m,
               torch::Tensor v, torch::Tensor state, double lr, double b1,
               double b2, double eps, double gscale = 1.0) {
  CHECK_IN(p); CHECK_IN(g); CHECK_IN(m); CHECK_IN(v); CHECK_IN(state);
  launch_adam(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
              v.data_ptr<float>(), state.data_ptr<float>(), p.numel(),
              (float)lr, (float)b1, (float)b2, (float)eps, (float)gscale, cur_stream());
}

// Adam with device-side dynamic loss scaling (sstate = [scale, clean-step
// counter, found_inf]): scans the flat grad for non-finites, skips the
// whole update on overflow, and adjusts the scale — all on device, so the
// captured step replays with the scale evolving (GradScaler semantics).
void adam_step_dynamic(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                       torch::Tensor v, torch::Tensor state,
                       torch::Tensor sstate, double lr, double b1, double b2,
                       double eps, double backoff, double growth,
                       double growth_interval) {
  CHECK_IN(p); CHECK_IN(g); CHECK_IN(m); CHECK_IN(v); CHECK_IN(state);
  CHECK_IN(sstate);
  TORCH_CHECK(sstate.numel() >= 3, "scaler state needs 3 elements");
  launch_adam_dynamic(p.data_ptr<float>(), g.data_ptr<float>(),
                      m.data_ptr<float>(), v.data_ptr<float>(),
                      state.data_ptr<float>(), sstate.data_ptr<float>(),
                      p.numel(), (float)lr, (float)b1, (float)b2, (float)eps,
                      (float)backoff, (float)growth, (float)growth_interval,
                      cur_stream());
}

// Extended Adam step: global-norm clipping (max_norm = inf: none), decoupled
// weight decay where decay_mask (uint8 per element) is set, and the learning
// rate of step t from lr_table[min(t, T) - 1].  hstate (8 floats) receives
// the rate, the clip coefficient and the norm statistics; slab is scratch
// for the norm's per-block partial sums.  sstate switches on the dynamic
// loss scaler as in adam_step_dynamic; without it gscale unscales.
void adam_step_ex(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                  torch::Tensor v, torch::Tensor state, OptTensor sstate,
                  torch::Tensor hstate, torch::Tensor slab,
                  OptTensor decay_mask, OptTensor lr_table, double lr,
                  double b1, double b2, double eps, double gscale, double wd,
                  double max_norm, double backoff, double growth,
                  double interval) {
  CHECK_IN(p); CHECK_IN(g); CHECK_IN(m); CHECK_IN(v); CHECK_IN(state);
  CHECK_IN(hstate); CHECK_IN(slab);
  const long numel = p.numel();
  TORCH_CHECK(g.numel() == numel && m.numel() == numel && v.numel() == numel,
              "p, g, m and v must have the same number of elements");
  TORCH_CHECK(state.numel() >= 3, "adam state needs 3 elements");
  TORCH_CHECK(hstate.numel() >= 8, "hstate needs 8 elements");
  TORCH_CHECK(slab.numel() >= 1, "slab needs at least 1 element");
  TORCH_CHECK(!(max_norm < 0.0) && max_norm == max_norm,
              "max_norm must be non-negative");
  float* ss = nullptr;
  if (sstate.has_value()) {
    CHECK_IN(*sstate);
    TORCH_CHECK(sstate->numel() >= 3, "scaler state needs 3 elements");
    ss = sstate->data_ptr<float>();
  }
  const unsigned char* mask = nullptr;
  if (decay_mask.has_value()) {
    CHECK_IN(*decay_mask);
    TORCH_CHECK(decay_mask->scalar_type() == torch::kUInt8 &&
                    decay_mask->numel() == numel,
                "decay_mask must be uint8 with one entry per element");
    mask = decay_mask->data_ptr<unsigned char>();
  }
  const float* table = nullptr;
  long table_len = 0;
  if (lr_table.has_value()) {
    CHECK_IN(*lr_table);
    table_len = lr_table->numel();
    TORCH_CHECK(table_len >= 1, "lr_table must not be empty");
    table = lr_table->data_ptr<float>();
  }
  launch_adam_ex(p.data_ptr<float>(), g.data_ptr<float>(),
                 m.data_ptr<float>(), v.data_ptr<float>(),
                 state.data_ptr<float>(), ss, hstate.data_ptr<float>(),
                 slab.data_ptr<float>(),
                 (int)std::min<long>(slab.numel(), 4096), mask, table,
                 table_len, numel, (float)lr, (float)b1, (float)b2,
                 (float)eps, (float)gscale, (float)wd, (float)max_norm,
                 (float)backoff, (float)growth, (float)interval,
                 cur_stream());
}

// ---------------------------------------------------------------------------
// Linear layers: y = x . w^T + b with x [m, k], w [n, k] (torch Linear
// layout), g = dy [m, n]; dgrad dx = g . w, wgrad dw = g^T . x, db = column
// sums of g.  Three families by the dtype of the activation streams:
//   fp32-IO  linear_fwd* / linear_bwd* / linear_dgrad / linear_wgrad / gemm_*
//   o16      linear_fwd_bf16_o16 / linear_dgrad16 / linear_wgrad16
//   a16      linear_fwd_a16o16[_wt] / linear_dgrad16_o16 / linear_wgrad16_b16
// ---------------------------------------------------------------------------

enum LinOp { LIN_FWD, LIN_DGRAD, LIN_WGRAD };
struct Mnk {
  int m, n, k;
};

// The one shape and dtype gate of every linear binding.  The operands are
// (x, w) forward, (g, w) dgrad and (g, x) wgrad, each of the dtype its family
// requires; the launchers take int extents and trust that the operands agree,
// so a mismatch stops here.  `bias`, where one is given (defined and not
// empty), holds n fp32 elements.
static Mnk linear_gate(const char* name, LinOp op, const torch::Tensor& a,
                       at::ScalarType a_dtype, const torch::Tensor& b,
                       at::ScalarType b_dtype,
                       const torch::Tensor* bias = nullptr) {
  const char* an = op == LIN_FWD ? "x" : "g";
  const char* bn = op == LIN_WGRAD ? "x" : "w";
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2, name, ": ", an, " and ", bn,
              " must be 2-D, got ", a.sizes(), " and ", b.sizes());
  TORCH_CHECK(a.scalar_type() == a_dtype && b.scalar_type() == b_dtype, name,
              ": ", an, " must be ", a_dtype, " and ", bn, " ", b_dtype,
              ", got ", a.scalar_type(), " and ", b.scalar_type());
  TORCH_CHECK(a.is_cuda() && a.device() == b.device(), name, ": ", an, " and ",
              bn, " must be on the same GPU");
  TORCH_CHECK(a.is_contiguous() && b.is_contiguous(), name, ": ", an, " and ",
              bn, " must be contiguous");
  int64_t m, n, k;
  if (op == LIN_FWD) {  // x [m, k], w [n, k]
    m = a.size(0), k = a.size(1), n = b.size(0);
    TORCH_CHECK(b.size(1) == k, name, ": w is ", b.sizes(), " but x ",
                a.sizes(), " has ", k, " columns");
  } else if (op == LIN_DGRAD) {  // g [m, n], w [n, k]
    m = a.size(0), n = b.size(0), k = b.size(1);
    TORCH_CHECK(a.size(1) == n, name, ": g is ", a.sizes(), " but w ",
                b.sizes(), " has ", n, " rows");
  } else {  // g [m, n], x [m, k]
    m = b.size(0), k = b.size(1), n = a.size(1);
    TORCH_CHECK(a.size(0) == m, name, ": g is ", a.sizes(), " but x ",
                b.sizes(), " has ", m, " rows");
  }
  TORCH_CHECK(m <= INT_MAX && n <= INT_MAX && k <= INT_MAX, name,
              ": an extent of [", m, ", ", n, ", ", k, "] does not fit an int");
  if (bias && bias->defined() && bias->numel() > 0)
    TORCH_CHECK(bias->scalar_type() == torch::kFloat32 && bias->numel() == n &&
                    bias->device() == a.device() && bias->is_contiguous(),
                name, ": the bias must be ", n, " contiguous fp32 elements on "
                "the operands' GPU, got ", bias->scalar_type(), " ",
                bias->sizes());
  return {(int)m, (int)n, (int)k};
}

static const float* bias_ptr(const torch::Tensor& b) {
  return b.defined() && b.numel() > 0 ? b.data_ptr<float>() : nullptr;
}

// The fp32-IO launchers by compute precision: prec 0 = fp32, 1 = bf16 and
// 2 = fp16 operands in the matrix cores (fp32 accumulate and output)
struct GemmF32io {
  decltype(&launch_gemm_f32_nt) nt;
  decltype(&launch_gemm_f32_nn) nn;
  decltype(&launch_gemm_f32_tn) tn;
};
static const GemmF32io& gemm_f32io(const char* name, int64_t prec) {
  static const GemmF32io table[3] = {
      {launch_gemm_f32_nt, launch_gemm_f32_nn, launch_gemm_f32_tn},
      {launch_gemm_bf16_nt, launch_gemm_bf16_nn, launch_gemm_bf16_tn},
      {launch_gemm_fp16_nt, launch_gemm_fp16_nn, launch_gemm_fp16_tn}};
  TORCH_CHECK(prec >= 0 && prec <= 2, name,
              ": prec must be 0 (fp32), 1 (bf16) or 2 (fp16), got ", prec);
  return table[prec];
}

static torch::Tensor linear_fwd_f32io(const char* name, int64_t prec,
                                      const torch::Tensor& x,
                                      const torch::Tensor& w,
                                      const torch::Tensor& b) {
  const auto& gemm = gemm_f32io(name, prec);
  const auto [m, n, k] = linear_gate(name, LIN_FWD, x, torch::kFloat32, w,
                                     torch::kFloat32, &b);
  auto y = torch::empty({m, n}, x.options());
  if (m == 0) return y;  // no rows: nothing to launch
  gemm.nt(x.data_ptr<float>(), w.data_ptr<float>(), bias_ptr(b),
          y.data_ptr<float>(), m, n, k, false, cur_stream());
  return y;
}

static torch::Tensor linear_dgrad_f32io(const char* name, int64_t prec,
                                        const torch::Tensor& g,
                                        const torch::Tensor& w) {
  const auto& gemm = gemm_f32io(name, prec);
  const auto [m, n, k] = linear_gate(name, LIN_DGRAD, g, torch::kFloat32, w,
                                     torch::kFloat32);
  auto dx = torch::empty({m, k}, g.options());
  if (m == 0) return dx;  // no rows: nothing to launch
  gemm.nn(g.data_ptr<float>(), w.data_ptr<float>(), nullptr,
          dx.data_ptr<float>(), m, n, k, false, cur_stream());
  return dx;
}

// -> {dw [n, k], db [n] or [0]}
static std::vector<torch::Tensor> linear_wgrad_f32io(const char* name,
                                                     int64_t prec,
                                                     const torch::Tensor& g,
                                                     const torch::Tensor& x,
                                                     bool has_bias) {
  const auto& gemm = gemm_f32io(name, prec);
  const auto [m, n, k] = linear_gate(name, LIN_WGRAD, g, torch::kFloat32, x,
                                     torch::kFloat32);
  if (m == 0)  // no rows: the sums over them are zero, nothing to launch
    return {torch::zeros({n, k}, x.options()),
            torch::zeros({has_bias ? n : 0}, g.options())};
  auto dw = torch::empty({n, k}, x.options());
  auto db = torch::empty({has_bias ? n : 0}, g.options());
  gemm.tn(g.data_ptr<float>(), x.data_ptr<float>(), dw.data_ptr<float>(),
          has_bias ? db.data_ptr<float>() : nullptr, m, n, k, cur_stream());
  return {dw, db};
}

// The raw GEMMs (tests / future fused paths) are the linear ops without a
// bias: gemm_nt(a, b) = a . b^T, gemm_nn(a, b) = a . b, gemm_tn(a, b) =
// a^T . b (zeros for an empty contraction)
static torch::Tensor gemm_raw_f32io(const char* name, LinOp op, int64_t prec,
                                    const torch::Tensor& a,
                                    const torch::Tensor& b) {
  if (op == LIN_FWD) return linear_fwd_f32io(name, prec, a, b, {});
  if (op == LIN_DGRAD) return linear_dgrad_f32io(name, prec, a, b);
  return linear_wgrad_f32io(name, prec, a, b, false)[0];
}

// dgrad, then wgrad: -> {dx, dw, db}.  x against w and g against x are
// checked here and g against w by the dgrad, so all three agree before the
// first launch.
static std::vector<torch::Tensor> linear_bwd_f32io(const char* name,
                                                   int64_t prec,
                                                   const torch::Tensor& g,
                                                   const torch::Tensor& x,
                                                   const torch::Tensor& w,
                                                   bool has_bias) {
  linear_gate(name, LIN_FWD, x, torch::kFloat32, w, torch::kFloat32);
  linear_gate(name, LIN_WGRAD, g, torch::kFloat32, x, torch::kFloat32);
  auto dx = linear_dgrad_f32io(name, prec, g, w);
  auto dwb = linear_wgrad_f32io(name, prec, g, x, has_bias);
  return {dx, dwb[0], dwb[1]};
}

using TensorList = std::vector<torch::Tensor>;
torch::Tensor linear_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor b) {
  return linear_fwd_f32io("linear_fwd", 0, x, w, b);
}
torch::Tensor linear_fwd_bf16(torch::Tensor x, torch::Tensor w,
                              torch::Tensor b) {
  return linear_fwd_f32io("linear_fwd_bf16", 1, x, w, b);
}
torch::Tensor linear_fwd_fp16(torch::Tensor x, torch::Tensor w,
                              torch::Tensor b) {
  return linear_fwd_f32io("linear_fwd_fp16", 2, x, w, b);
}
TensorList linear_bwd(torch::Tensor g, torch::Tensor x, torch::Tensor w,
                   bool has_bias) {
  return linear_bwd_f32io("linear_bwd", 0, g, x, w, has_bias);
}
TensorList linear_bwd_bf16(torch::Tensor g, torch::Tensor x, torch::Tensor w,
                        bool has_bias) {
  return linear_bwd_f32io("linear_bwd_bf16", 1, g, x, w, has_bias);
}
TensorList linear_bwd_fp16(torch::Tensor g, torch::Tensor x, torch::Tensor w,
                        bool has_bias) {
  return linear_bwd_f32io("linear_bwd_fp16", 2, g, x, w, has_bias);
}
// split backward entry points so python can overlap dgrad (current stream)
// with wgrad+bias-grad (side stream)
torch::Tensor linear_dgrad(torch::Tensor g, torch::Tensor w, int64_t prec) {
  return linear_dgrad_f32io("linear_dgrad", prec, g, w);
}
TensorList linear_wgrad(torch::Tensor g, torch::Tensor x, bool has_bias,
                     int64_t prec) {
  return linear_wgrad_f32io("linear_wgrad", prec, g, x, has_bias);
}
torch::Tensor gemm_nt(torch::Tensor a, torch::Tensor b) {
  return gemm_raw_f32io("gemm_nt", LIN_FWD, 0, a, b);
}
torch::Tensor gemm_nn(torch::Tensor a, torch::Tensor b) {
  return gemm_raw_f32io("gemm_nn", LIN_DGRAD, 0, a, b);
}
torch::Tensor gemm_tn(torch::Tensor a, torch::Tensor b) {
  return gemm_raw_f32io("gemm_tn", LIN_WGRAD, 0, a, b);
}
torch::Tensor gemm_nt_bf16(torch::Tensor a, torch::Tensor b) {
  return gemm_raw_f32io("gemm_nt_bf16", LIN_FWD, 1, a, b);
}
torch::Tensor gemm_nn_bf16(torch::Tensor a, torch::Tensor b) {
  return gemm_raw_f32io("gemm_nn_bf16", LIN_DGRAD, 1, a, b);
}
torch::Tensor gemm_tn_bf16(torch::Tensor a, torch::Tensor b) {
  return gemm_raw_f32io("gemm_tn_bf16", LIN_WGRAD, 1, a, b);
}

// dtable[r] = sum over g rows whose table index is r; order/ptr group the
// g-row indices by table row (deterministic, no atomics).
torch::Tensor embed_grouped_scatter(torch::Tensor g, torch::Tensor order,
                                    torch::Tensor ptr, int64_t rows,
                                    int64_t h, int64_t col_off) {
  CHECK_IN(g); CHECK_IN(order); CHECK_IN(ptr);
  const long num_src = order.size(0);
  // sub-waves per row: target ~16k waves to hide gather latency across the
  // whole chip, but never more sub-waves than a row could populate
  long p = 16384 / std::max<int64_t>(rows, 1);
  const long per_row = (num_src + std::max<int64_t>(rows, 1) - 1) /
                       std::max<int64_t>(rows, 1);
  p = std::min<long>(p, per_row);
  p = std::min<long>(std::max<long>(p, 1), 256);
  auto dtable = torch::empty({rows, h}, g.options());
  auto partial = torch::empty({rows * p, h}, g.options());
  launch_embed_grouped_scatter(g.data_ptr<float>(), order.data_ptr<int>(),
                               ptr.data_ptr<int>(), partial.data_ptr<float>(),
                               dtable.data_ptr<float>(), num_src, (int)rows,
                               (int)p, (int)h, (int)g.size(1), (int)col_off,
                               cur_stream());
  return dtable;
}

// Work-balanced deterministic grouped scatter: waves assigned per row in
// proportion to its group size (row_map/wave_start built host-side at
// _group_by time) — robust to the PERT interface-0 mega-group (quirk 6).
torch::Tensor embed_grouped_scatter_bal(torch::Tensor g, torch::Tensor order,
                                        torch::Tensor ptr,
                                        torch::Tensor row_map,
                                        torch::Tensor wave_start,
                                        torch::Tensor row_map2,
                                        torch::Tensor wave_start2,
                                        int64_t rows, int64_t h,
                                        int64_t col_off) {
  CHECK_IN(g); CHECK_IN(order); CHECK_IN(ptr);
  CHECK_IN(row_map); CHECK_IN(wave_start);
  TORCH_CHECK(wave_start.numel() == rows + 1,
              "wave_start must have rows+1 entries");
  const int n_waves = row_map.size(0);
  const int n_waves2 = row_map2.size(0);  // 0 => single-level fold
  const int g16 = g.scalar_type() == torch::kBFloat16 ? 1 : 0;
  auto fopt = g.options().dtype(torch::kFloat32);
  auto dtable = torch::empty({rows, h}, fopt);
  auto partial = torch::empty({(long)n_waves, h}, fopt);
  auto partial2 = torch::empty({(long)n_waves2, h}, fopt);
  launch_embed_grouped_scatter_bal(
      g.data_ptr(), g16, order.data_ptr<int>(), ptr.data_ptr<int>(),
      row_map.data_ptr<int>(), wave_start.data_ptr<int>(),
      n_waves2 ? row_map2.data_ptr<int>() : nullptr,
      n_waves2 ? wave_start2.data_ptr<int>() : nullptr,
      partial.data_ptr<float>(), partial2.data_ptr<float>(),
      dtable.data_ptr<float>(), n_waves, n_waves2,
      (int)rows, (int)h, (int)g.size(1), (int)col_off, cur_stream());
  return dtable;
}

// Both P-table gradients from one pass over de [E, h]: out[:V] = dP_ifc,
// out[V:] = dP_rpc.  The six plan tensors (int32; built and validated by
// edge_table_plan in pertgnn/ops/functional.py) are three levels of row
// lists: chunks of equal (ifc, rpc) key over the edges, groups over the
// members of every over-long table row, one list per table row.  Three
// launches of one kernel (two when there is no level 2): no memset, no
// atomics, the final rows rounded once into out_dtype.
torch::Tensor edge_table_grad(torch::Tensor de, torch::Tensor idx1,
                              torch::Tensor lptr1, torch::Tensor idx2,
                              torch::Tensor lptr2, torch::Tensor idx3,
                              torch::Tensor lptr3, int64_t V, int64_t R,
                              at::ScalarType out_dtype, int64_t unroll = 8) {
  CHECK_IN(de); CHECK_IN(idx1); CHECK_IN(lptr1); CHECK_IN(idx2);
  CHECK_IN(lptr2); CHECK_IN(idx3); CHECK_IN(lptr3);
  TORCH_CHECK(de.dim() == 2, "de must be [E, h]");
  TORCH_CHECK(de.scalar_type() == torch::kBFloat16 ||
                  de.scalar_type() == torch::kFloat32,
              "de must be bf16 or fp32");
  TORCH_CHECK(out_dtype == torch::kBFloat16 || out_dtype == torch::kFloat32,
              "out_dtype must be bf16 or fp32");
  for (const auto& t : {idx1, lptr1, idx2, lptr2, idx3, lptr3})
    TORCH_CHECK(t.scalar_type() == torch::kInt32 && t.dim() == 1,
                "plan tensors must be 1-D int32");
  TORCH_CHECK(V >= 0 && R >= 0 && lptr3.numel() == V + R + 1,
              "lptr3 must have V+R+1 entries");
  TORCH_CHECK(lptr1.numel() >= 1 && lptr2.numel() >= 1,
              "lptr1/lptr2 must have at least one entry");
  TORCH_CHECK(idx1.numel() == de.size(0),
              "level 1 must list every row of de exactly once");
  const int h = (int)de.size(1);
  const long n1 = lptr1.numel() - 1;
  const long n2 = lptr2.numel() - 1;
  const int in16 = de.scalar_type() == torch::kBFloat16 ? 1 : 0;
  const int out16 = out_dtype == torch::kBFloat16 ? 1 : 0;
  auto partial =
      torch::empty({n1 + n2, (long)h}, de.options().dtype(torch::kFloat32));
  auto out = torch::empty({V + R, (long)h}, de.options().dtype(out_dtype));
  hipStream_t s = cur_stream();
  launch_rows_sum_lists(de.data_ptr(), in16, idx1.data_ptr<int>(),
                        lptr1.data_ptr<int>(), partial.data_ptr(), 0, (int)n1,
                        h, (int)unroll, s);
  if (n2 > 0)
    launch_rows_sum_lists(partial.data_ptr(), 0, idx2.data_ptr<int>(),
                          lptr2.data_ptr<int>(),
                          partial.data_ptr<float>() + n1 * h, 0, (int)n2, h,
                          (int)unroll, s);
  launch_rows_sum_lists(partial.data_ptr(), 0, idx3.data_ptr<int>(),
                        lptr3.data_ptr<int>(), out.data_ptr(), out16,
                        (int)(V + R), h, (int)unroll, s);
  return out;
}

// The category-table gradient of the first layer without its dgrad GEMM:
// dtable[rows, h] = G . B, where G[c, :] is the sum of the dqkvs rows
// [n, 4h] (bf16) of category c and B[j, t] = bf16(w4[j, f + t]) are the
// table's columns of the layer's fp32 weight [4h, k_padded], rounded as the
// dgrad GEMM rounds them.  The six plan tensors (cat_table_plan in
// pertgnn/ops/functional.py, one key) drive three launches of the wide list
// sum (two without a level 2) over all 4h columns, fp32 in list order; the
// small fp32 GEMM then stores dtable, or adds it into `sink` and returns an
// empty tensor.  No [n, .] intermediate, no memset, no atomics.  n == 0:
// zeros (the sink untouched), nothing launched.
torch::Tensor embed_dgrad_fold(torch::Tensor dqkvs, torch::Tensor idx1,
                               torch::Tensor lptr1, torch::Tensor idx2,
                               torch::Tensor lptr2, torch::Tensor idx3,
                               torch::Tensor lptr3, torch::Tensor w4,
                               int64_t f, int64_t h, int64_t rows,
                               OptTensor sink = std::nullopt,
                               int64_t unroll = 8, int64_t seg_cols = 256) {
  CHECK_IN(dqkvs); CHECK_IN(idx1); CHECK_IN(lptr1); CHECK_IN(idx2);
  CHECK_IN(lptr2); CHECK_IN(idx3); CHECK_IN(lptr3); CHECK_IN(w4);
  TORCH_CHECK(h == 256 || h == 512, "embed_dgrad_fold: h must be 256 or 512");
  TORCH_CHECK(dqkvs.dim() == 2 && dqkvs.size(1) == 4 * h &&
                  dqkvs.scalar_type() == torch::kBFloat16,
              "embed_dgrad_fold: dqkvs must be bf16 [n, 4h]");
  TORCH_CHECK(w4.dim() == 2 && w4.size(0) == 4 * h &&
                  w4.scalar_type() == torch::kFloat32,
              "embed_dgrad_fold: w4 must be fp32 [4h, k_padded]");
  TORCH_CHECK(f >= 0 && f + h <= w4.size(1),
              "embed_dgrad_fold: columns f..f+h must lie inside w4");
  for (const auto& t : {idx1, lptr1, idx2, lptr2, idx3, lptr3})
    TORCH_CHECK(t.scalar_type() == torch::kInt32 && t.dim() == 1,
                "plan tensors must be 1-D int32");
  TORCH_CHECK(rows >= 0 && lptr3.numel() == rows + 1,
              "embed_dgrad_fold: lptr3 must have rows+1 entries");
  TORCH_CHECK(lptr1.numel() >= 1 && lptr2.numel() >= 1,
              "lptr1/lptr2 must have at least one entry");
  TORCH_CHECK(idx1.numel() == dqkvs.size(0),
              "level 1 must list every row of dqkvs exactly once");
  float* sink_p = grad_sink(sink, dqkvs, {rows, h}, "embed_dgrad_fold");
  auto fopt = dqkvs.options().dtype(torch::kFloat32);
  if (dqkvs.size(0) == 0 || rows == 0)
    return sink_p ? torch::empty({0}, fopt) : torch::zeros({rows, h}, fopt);
  const int width = (int)(4 * h);
  const long n1 = lptr1.numel() - 1;
  const long n2 = lptr2.numel() - 1;
  // level-1 rows, level-2 rows, then G
  auto buf = torch::empty({n1 + n2 + rows, (long)width}, fopt);
  float* p = buf.data_ptr<float>();
  float* G = p + (n1 + n2) * width;
  hipStream_t s = cur_stream();
  launch_rows_sum_lists_wide(dqkvs.data_ptr(), 1, width, idx1.data_ptr<int>(),
                             lptr1.data_ptr<int>(), p, width, (int)n1, width,
                             (int)seg_cols, (int)unroll, s);
  if (n2 > 0)
    launch_rows_sum_lists_wide(p, 0, width, idx2.data_ptr<int>(),
                               lptr2.data_ptr<int>(), p + n1 * width, width,
                               (int)n2, width, (int)seg_cols, (int)unroll, s);
  launch_rows_sum_lists_wide(p, 0, width, idx3.data_ptr<int>(),
                             lptr3.data_ptr<int>(), G, width, (int)rows, width,
                             (int)seg_cols, (int)unroll, s);
  auto out = torch::empty({sink_p ? 0 : rows, sink_p ? 0 : h}, fopt);
  launch_embed_fold_gemm(G, w4.data_ptr<float>(),
                         sink_p ? sink_p : out.data_ptr<float>(), (int)rows,
                         width, (int)h, (int)w4.size(1), (int)f,
                         sink_p != nullptr, s);
  return out;
}

// ---------------------------------------------------------------------------
// Fused edge attention over qkvs [N, 4h] (fp32 or bf16), the two P tables
// (fp32, or bf16 with bf16 qkvs), edge_attr [E, >=2] and the CSR arrays.
// ---------------------------------------------------------------------------

struct AttnShape {
  int n, h;
  long ne;
  bool b16, p16;  // bf16 qkvs / bf16 P tables
};

// The checks every fused-attention binding shares (the forward half)
static AttnShape attn_gate(const char* name, const torch::Tensor& qkvs,
                           const torch::Tensor& pifc,
                           const torch::Tensor& prpc, const torch::Tensor& ea,
                           const torch::Tensor& row_ptr,
                           const torch::Tensor& csr_src, int64_t heads) {
  for (const auto* t : {&qkvs, &pifc, &prpc, &ea, &row_ptr, &csr_src})
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                    t->device() == qkvs.device(),
                name, ": every operand must be contiguous and on one GPU");
  TORCH_CHECK(qkvs.dim() == 2 && qkvs.size(1) % 4 == 0 &&
                  qkvs.size(0) <= INT_MAX,
              name, ": qkvs must be [N, 4h]");
  AttnShape s;
  s.n = (int)qkvs.size(0);
  s.h = (int)(qkvs.size(1) / 4);
  s.ne = ea.size(0);
  s.b16 = qkvs.scalar_type() == torch::kBFloat16;
  s.p16 = pifc.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(s.h <= 512, name, ": H must be <= 512");
  TORCH_CHECK(heads >= 1 && heads <= s.h && s.h % heads == 0, name,
              ": heads must divide H (H=", s.h, ", heads=", heads, ")");
  TORCH_CHECK(s.b16 || qkvs.scalar_type() == torch::kFloat32, name,
              ": qkvs must be fp32 or bf16");
  TORCH_CHECK(!s.p16 || s.b16, name, ": bf16 P tables require bf16 qkvs");
  TORCH_CHECK(pifc.scalar_type() == prpc.scalar_type(), name,
              ": P tables must share a dtype");
  TORCH_CHECK(s.p16 || pifc.scalar_type() == torch::kFloat32, name,
              ": P tables must be fp32 or bf16");
  TORCH_CHECK(pifc.dim() == 2 && prpc.dim() == 2 && pifc.size(1) == s.h &&
                  prpc.size(1) == s.h,
              name, ": P tables must have width h");
  TORCH_CHECK(ea.dim() == 2 && ea.size(1) >= 2 &&
                  ea.scalar_type() == torch::kLong,
              name, ": edge_attr must be int64 [E, >=2]");
  TORCH_CHECK(row_ptr.scalar_type() == torch::kInt32 &&
                  csr_src.scalar_type() == torch::kInt32 &&
                  row_ptr.numel() == (int64_t)s.n + 1 &&
                  csr_src.numel() == s.ne,
              name, ": CSR arrays (int32) do not match qkvs/edge_attr");
  return s;
}

// The backward, shared by edge_attn_fused_bwd, edge_attn_bn_bwd16 and
// edge_attn_pool_bwd16.  Constructing it checks the operands (the forward's
// checks, alpha of the forward, the CSC arrays, and g [n, h] where there is
// one: the pool mode forms it itself), so a binding can launch what must
// precede the attention kernels in between; run() allocates {dqkvs, de} and
// launches.  The softmax backward is single-pass: no [E, h] dek/dev scratch,
// the col kernel regenerates the rank-1 per-edge grads from the per-edge
// scalars (dal = logit grad, alpha) and row gathers of q/g.
struct AttnBwd {
  const torch::Tensor *g, &qkvs, &pifc, &prpc, &ea, &alpha, &row_ptr, &csr_src,
      &col_ptr, &csc_dst, &csc_eid;
  const int64_t heads;
  const AttnShape s;

  AttnBwd(const char* name, const torch::Tensor* g, const torch::Tensor& qkvs,
          const torch::Tensor& pifc, const torch::Tensor& prpc,
          const torch::Tensor& ea, const torch::Tensor& alpha,
          const torch::Tensor& row_ptr, const torch::Tensor& csr_src,
          const torch::Tensor& col_ptr, const torch::Tensor& csc_dst,
          const torch::Tensor& csc_eid, int64_t heads)
      : g(g), qkvs(qkvs), pifc(pifc), prpc(prpc), ea(ea), alpha(alpha),
        row_ptr(row_ptr), csr_src(csr_src), col_ptr(col_ptr), csc_dst(csc_dst),
        csc_eid(csc_eid), heads(heads),
        s(attn_gate(name, qkvs, pifc, prpc, ea, row_ptr, csr_src, heads)) {
    for (const auto* t : {&alpha, &col_ptr, &csc_dst, &csc_eid})
      TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                      t->device() == qkvs.device(),
                  name, ": every operand must be contiguous and on one GPU");
    TORCH_CHECK(alpha.scalar_type() == torch::kFloat32 &&
                    alpha.numel() == s.ne * heads,
                name,
                ": alpha must be the fp32 [E, heads] tensor of the forward");
    TORCH_CHECK(col_ptr.scalar_type() == torch::kInt32 &&
                    csc_dst.scalar_type() == torch::kInt32 &&
                    csc_eid.scalar_type() == torch::kInt32 &&
                    col_ptr.numel() == (int64_t)s.n + 1 &&
                    csc_dst.numel() == s.ne && csc_eid.numel() == s.ne,
                name, ": CSC arrays (int32) do not match qkvs/edge_attr");
    TORCH_CHECK(g || s.b16, name, " takes bf16 qkvs");
    if (g)
      TORCH_CHECK(g->is_cuda() && g->is_contiguous() && g->dim() == 2 &&
                      g->size(0) == s.n && g->size(1) == s.h &&
                      (g->scalar_type() == torch::kFloat32 ||
                       (s.b16 && g->scalar_type() == torch::kBFloat16)),
                  name, ": g must be [n, h], fp32 (or bf16 with bf16 qkvs)");
  }

  // bn / pool (bf16 qkvs only) as in launch_edge_attn_fused_bwd16
  std::vector<torch::Tensor> run(const AttnBnBwd* bn = nullptr,
                                 const AttnPoolBwd* pool = nullptr) const {
    auto fopt = qkvs.options().dtype(torch::kFloat32);
    auto dqkvs = torch::empty_like(qkvs);
    // edge scratch matches qkvs dtype
    auto de = torch::empty({s.ne, s.h}, s.b16 ? qkvs.options() : fopt);
    auto dal = torch::empty({s.ne * heads}, fopt);  // [E, heads] row-major
    if (s.b16) {
      const int g16 = g && g->scalar_type() == torch::kBFloat16 ? 1 : 0;
      launch_edge_attn_fused_bwd16(
          g ? g->data_ptr() : nullptr, g16, qkvs.data_ptr(), pifc.data_ptr(),
          prpc.data_ptr(), s.p16 ? 1 : 0, ea.data_ptr<long>(),
          (int)ea.size(1), alpha.data_ptr<float>(), row_ptr.data_ptr<int>(),
          csr_src.data_ptr<int>(), col_ptr.data_ptr<int>(),
          csc_dst.data_ptr<int>(), csc_eid.data_ptr<int>(), dqkvs.data_ptr(),
          de.data_ptr(), dal.data_ptr<float>(), s.n, s.h, s.ne, (int)heads,
          cur_stream(), bn, pool);
    } else {
      TORCH_CHECK(!bn && !pool, "the fused BN / pool backward needs bf16 qkvs");
      launch_edge_attn_fused_bwd(
          g->data_ptr<float>(), qkvs.data_ptr<float>(),
          pifc.data_ptr<float>(), prpc.data_ptr<float>(), ea.data_ptr<long>(),
          (int)ea.size(1), alpha.data_ptr<float>(), row_ptr.data_ptr<int>(),
          csr_src.data_ptr<int>(), col_ptr.data_ptr<int>(),
          csc_dst.data_ptr<int>(), csc_eid.data_ptr<int>(),
          dqkvs.data_ptr<float>(), de.data_ptr<float>(),
          dal.data_ptr<float>(), s.n, s.h, s.ne, (int)heads, cur_stream());
    }
    return {dqkvs, de};
  }
};

std::vector<torch::Tensor> edge_attn_fused_fwd(
    torch::Tensor qkvs, torch::Tensor pifc, torch::Tensor prpc,
    torch::Tensor ea, torch::Tensor row_ptr, torch::Tensor csr_src,
    bool out16, int64_t heads = 1) {
  const auto [n, h, ne, b16, p16] = attn_gate(
      "edge_attn_fused_fwd", qkvs, pifc, prpc, ea, row_ptr, csr_src, heads);
  TORCH_CHECK(!out16 || b16, "edge_attn_fused_fwd: out16 requires bf16 qkvs");
  auto fopt = qkvs.options().dtype(torch::kFloat32);
  auto out = torch::empty({n, h}, out16 ? qkvs.options() : fopt);
  // per-(edge, head) attention weights: [E] single-head, [E, heads] otherwise
  auto alpha = heads == 1 ? torch::empty({ea.size(0)}, fopt)
                          : torch::empty({ea.size(0), heads}, fopt);
  if (b16) {
    launch_edge_attn_fused_fwd16(
        qkvs.data_ptr(), pifc.data_ptr(), prpc.data_ptr(), p16 ? 1 : 0,
        ea.data_ptr<long>(), (int)ea.size(1),
        row_ptr.data_ptr<int>(), csr_src.data_ptr<int>(),
        out.data_ptr(), out16 ? 1 : 0, alpha.data_ptr<float>(), n, h,
        (int)heads, cur_stream());
  } else {
    launch_edge_attn_fused_fwd(
        qkvs.data_ptr<float>(), pifc.data_ptr<float>(), prpc.data_ptr<float>(),
        ea.data_ptr<long>(), (int)ea.size(1), row_ptr.data_ptr<int>(),
        csr_src.data_ptr<int>(), out.data_ptr<float>(), alpha.data_ptr<float>(),
        n, h, (int)heads, cur_stream());
  }
  return {out, alpha};
}

// Forward-only fused attention for inference: no alpha, and the eval-mode
// BatchNorm folded to a per-channel affine (bn_scale/bn_shift, fp32 [h];
// both empty = no affine) plus the optional ReLU applied in the kernel's
// epilogue before the single store.
torch::Tensor edge_attn_fused_infer(
    torch::Tensor qkvs, torch::Tensor pifc, torch::Tensor prpc,
    torch::Tensor ea, torch::Tensor row_ptr, torch::Tensor csr_src,
    torch::Tensor bn_scale, torch::Tensor bn_shift, bool relu, bool out16,
    int64_t heads = 1) {
  const auto [n, h, ne, b16, p16] = attn_gate(
      "edge_attn_fused_infer", qkvs, pifc, prpc, ea, row_ptr, csr_src, heads);
  TORCH_CHECK(!out16 || b16,
              "edge_attn_fused_infer: out16 requires bf16 qkvs");
  TORCH_CHECK(bn_scale.numel() == bn_shift.numel() &&
                  (bn_scale.numel() == 0 || bn_scale.numel() == h),
              "bn_scale/bn_shift must both be empty or both have h elements");
  const float* sc = nullptr;
  const float* sh = nullptr;
  if (bn_scale.numel() > 0) {
    TORCH_CHECK(bn_scale.scalar_type() == torch::kFloat32 &&
                    bn_shift.scalar_type() == torch::kFloat32,
                "bn_scale/bn_shift must be fp32");
    TORCH_CHECK(bn_scale.is_contiguous() && bn_shift.is_contiguous(),
                "bn_scale/bn_shift must be contiguous");
    TORCH_CHECK(bn_scale.device() == qkvs.device() &&
                    bn_shift.device() == qkvs.device(),
                "bn_scale/bn_shift must be on the device of qkvs");
    sc = bn_scale.data_ptr<float>();
    sh = bn_shift.data_ptr<float>();
  }
  auto fopt = qkvs.options().dtype(torch::kFloat32);
  auto out = torch::empty({n, h}, out16 ? qkvs.options() : fopt);
  if (b16) {
    launch_edge_attn_fused_infer16(
        qkvs.data_ptr(), pifc.data_ptr(), prpc.data_ptr(), p16 ? 1 : 0,
        ea.data_ptr<long>(), (int)ea.size(1), row_ptr.data_ptr<int>(),
        csr_src.data_ptr<int>(), sc, sh, relu ? 1 : 0, out.data_ptr(),
        out16 ? 1 : 0, n, h, (int)heads, cur_stream());
  } else {
    launch_edge_attn_fused_infer(
        qkvs.data_ptr<float>(), pifc.data_ptr<float>(), prpc.data_ptr<float>(),
        ea.data_ptr<long>(), (int)ea.size(1), row_ptr.data_ptr<int>(),
        csr_src.data_ptr<int>(), sc, sh, relu ? 1 : 0, out.data_ptr<float>(),
        n, h, (int)heads, cur_stream());
  }
  return out;
}

std::vector<torch::Tensor> edge_attn_fused_bwd(
    torch::Tensor g, torch::Tensor qkvs, torch::Tensor pifc,
    torch::Tensor prpc, torch::Tensor ea, torch::Tensor alpha,
    torch::Tensor row_ptr, torch::Tensor csr_src, torch::Tensor col_ptr,
    torch::Tensor csc_dst, torch::Tensor csc_eid, int64_t heads = 1) {
  return AttnBwd("edge_attn_fused_bwd", &g, qkvs, pifc, prpc, ea, alpha,
                 row_ptr, csr_src, col_ptr, csc_dst, csc_eid, heads)
      .run();
}

// dtable[v] += sum of g[r, col_off:col_off+h] over rows r with idx[r]==v.
// idx may be a strided column view of an [N,A] attr tensor.
torch::Tensor vocab_scatter(torch::Tensor g, torch::Tensor idx, int64_t rows,
                            int64_t h, int64_t col_off) {
  CHECK_IN(g);
  TORCH_CHECK(idx.is_cuda() && idx.dim() == 1, "idx must be 1-D CUDA");
  const size_t lds = (size_t)rows * h * sizeof(float);
  TORCH_CHECK(lds <= 160 * 1024, "vocab too large for LDS accumulator");
  auto dtable = torch::empty({rows, h}, g.options().dtype(torch::kFloat32));
  if (g.scalar_type() == torch::kBFloat16) {
    // wave-private kernel handles bf16 g directly when its tables fit
    const size_t priv64 = (size_t)4 * rows * 64 * sizeof(float);
    TORCH_CHECK(h % 64 == 0 && priv64 <= 160 * 1024,
                "bf16 vocab_scatter needs the wave-private path "
                "(upcast g to f32 for this shape)");
    launch_vocab_scatter16(g.data_ptr(), idx.data_ptr<long>(), idx.stride(0),
                           dtable.data_ptr<float>(), g.size(0), (int)rows,
                           (int)h, (int)g.size(1), (int)col_off,
                           cur_stream());
    return dtable;
  }
  launch_vocab_scatter(g.data_ptr<float>(), idx.data_ptr<long>(),
                       idx.stride(0), dtable.data_ptr<float>(), g.size(0),
                       (int)rows, (int)h, (int)g.size(1), (int)col_off,
                       cur_stream());
  return dtable;
}

// sync-BN partials: [2h+1] — per-channel sum / sum-of-squares plus the
// LOCAL row count in the tail slot, so a single all-reduce carries sums AND
// the global count with no host round-trip (SURVEY.md §7 hard part 4).
torch::Tensor bn_stats(torch::Tensor x) {
  CHECK_IN(x);
  const long h = x.size(1);
  auto partials = torch::empty({2 * h + 1},
                               x.options().dtype(torch::kFloat32));
  auto slab = bn_wide_slab(x);
  if (x.scalar_type() == torch::kBFloat16)
    launch_bn_stats_only16(x.data_ptr(), x.size(0), h,
                           partials.data_ptr<float>(), bn_slab_ptr(slab),
                           cur_stream());
  else
    launch_bn_stats_only(x.data_ptr<float>(), x.size(0), h,
                         partials.data_ptr<float>(), bn_slab_ptr(slab),
                         cur_stream());
  partials.narrow(0, 2 * h, 1).fill_((float)x.size(0));
  return partials;
}

// both dP tables in one pass over de (h % 256 == 0 required)
std::vector<torch::Tensor> vocab_scatter_dual(torch::Tensor g,
                                              torch::Tensor ea, int64_t rows0,
                                              int64_t rows1) {
  CHECK_IN(g); CHECK_IN(ea);
  const int h = g.size(1);
  TORCH_CHECK(h % 256 == 0, "dual scatter needs h % 256 == 0");
  TORCH_CHECK((size_t)(rows0 + rows1) * h * 4 <= 160 * 1024, "tables too large");
  auto fopt = g.options().dtype(torch::kFloat32);
  auto dt0 = torch::empty({rows0, h}, fopt);
  auto dt1 = torch::empty({rows1, h}, fopt);
  if (g.scalar_type() == torch::kBFloat16)
    launch_vocab_scatter_dual16(g.data_ptr(), ea.data_ptr<long>(),
                                (int)ea.size(1), dt0.data_ptr<float>(),
                                dt1.data_ptr<float>(), g.size(0), (int)rows0,
                                (int)rows1, h, cur_stream());
  else
    launch_vocab_scatter_dual(g.data_ptr<float>(), ea.data_ptr<long>(),
                              (int)ea.size(1), dt0.data_ptr<float>(),
                              dt1.data_ptr<float>(), g.size(0), (int)rows0,
                              (int)rows1, h, cur_stream());
  return {dt0, dt1};
}

// bf16-activation-mode linear: fp32 x/w in, bf16 C out; backward from bf16 g
torch::Tensor linear_fwd_bf16_o16(torch::Tensor x, torch::Tensor w,
                                  torch::Tensor b) {
  const auto [m, n, k] = linear_gate("linear_fwd_bf16_o16", LIN_FWD, x,
                                     torch::kFloat32, w, torch::kFloat32, &b);
  auto y = torch::empty({m, n}, x.options().dtype(torch::kBFloat16));
  if (m == 0) return y;  // no rows: nothing to launch
  launch_gemm_bf16_nt_o16(x.data_ptr<float>(), w.data_ptr<float>(),
                          bias_ptr(b), y.data_ptr(), m, n, k, cur_stream());
  return y;
}

torch::Tensor linear_dgrad16(torch::Tensor g, torch::Tensor w) {
  const auto [m, n, k] = linear_gate("linear_dgrad16", LIN_DGRAD, g,
                                     torch::kBFloat16, w, torch::kFloat32);
  auto dx = torch::empty({m, k}, w.options());
  if (m == 0) return dx;  // no rows: nothing to launch
  if (gemm_dispatch::dgrad_skinny(m)) {  // tiny-row P-table backward
    launch_gemm_skinny_nn(g.data_ptr(), w.data_ptr<float>(),
                          dx.data_ptr<float>(), m, n, k, cur_stream());
    return dx;
  }
  launch_gemm_bf16_nn_a16(g.data_ptr(),
                          w.data_ptr<float>(), dx.data_ptr<float>(), m, n, k,
                          cur_stream());
  return dx;
}

// dw_sink / db_sink (here and in linear_wgrad16_b16): gradient sinks of w
// and b.  With dw_sink the op adds dw (and db, whose sink must then come
// along when has_bias) into them and returns two empty tensors.
std::vector<torch::Tensor> linear_wgrad16(torch::Tensor g, torch::Tensor x,
                                          bool has_bias,
                                          OptTensor dw_sink = std::nullopt,
                                          OptTensor db_sink = std::nullopt,
                                          int64_t tile = 0) {
  // `tile` as in linear_wgrad16_b16; with fp32 x no shape reaches the glds
  // TN kernel, so none can be forced
  TORCH_CHECK(tile == 0, "linear_wgrad16: fp32 x does not run on the glds TN "
                         "kernel, no tile to force");
  const auto [m, n, k] = linear_gate("linear_wgrad16", LIN_WGRAD, g,
                                     torch::kBFloat16, x, torch::kFloat32);
  float* dw_s = grad_sink(dw_sink, x, {n, k}, "linear_wgrad16");
  float* db_s = grad_sink(db_sink, x, {n}, "linear_wgrad16");
  TORCH_CHECK((db_s != nullptr) == (dw_s != nullptr && has_bias),
              "linear_wgrad16: a db sink comes with a dw sink and a bias");
  if (dw_s) {
    if (m > 0)  // no rows: nothing to add
      launch_gemm_bf16_tn_a16(g.data_ptr(), x.data_ptr<float>(), dw_s, db_s, m,
                              n, k, cur_stream(), /*acc=*/true);
    return {torch::empty({0}, x.options()), torch::empty({0}, x.options())};
  }
  if (m == 0)  // no rows: the sums over them are zero, nothing to launch
    return {torch::zeros({n, k}, x.options()),
            torch::zeros({has_bias ? n : 0}, x.options())};
  auto dw = torch::empty({n, k}, x.options());
  torch::Tensor db = torch::empty({0}, x.options());
  float* db_ptr = nullptr;
  if (has_bias) {
    db = torch::empty({n}, x.options());
    db_ptr = db.data_ptr<float>();
  }
  launch_gemm_bf16_tn_a16(g.data_ptr(),
                          x.data_ptr<float>(), dw.data_ptr<float>(), db_ptr,
                          m, n, k, cur_stream());
  return {dw, db};
}


// ---------------------------------------------------------------------------
// act16-v2: bf16 activation streams between BN <-> GEMMs <-> pool.
// Statistics, affine params, weights and weight-grads stay fp32.
// ---------------------------------------------------------------------------

// Backward of "fused attention forward -> BN+ReLU(+dropout) forward" in act16
// mode: g is the gradient of the BN output, x the attention output the BN
// read, mask the BN forward's keep mask.  The BN partials run as in
// bn_relu_bwd16; the element-wise BN backward runs inside the attention
// backward's row kernel, so no [n, h] dx is allocated, written or re-read.
// Sync-BN passes the all-reduced [2h+1] partials (global count in the tail
// slot) and the local [2h+1] ones (dgamma/dbeta), as bn_bwd_apply16 takes
// them.  Returns {dqkvs, de, dgamma, dbeta}.
std::vector<torch::Tensor> edge_attn_bn_bwd16(
    torch::Tensor g, torch::Tensor x, torch::Tensor mask, torch::Tensor gamma,
    torch::Tensor mean, torch::Tensor invstd, double keep_inv,
    torch::Tensor qkvs, torch::Tensor pifc, torch::Tensor prpc,
    torch::Tensor ea, torch::Tensor alpha, torch::Tensor row_ptr,
    torch::Tensor csr_src, torch::Tensor col_ptr, torch::Tensor csc_dst,
    torch::Tensor csc_eid, int64_t heads = 1,
    std::optional<torch::Tensor> partials_global_opt = std::nullopt,
    std::optional<torch::Tensor> partials_local_opt = std::nullopt,
    OptTensor dgamma_sink = std::nullopt,
    OptTensor dbeta_sink = std::nullopt) {
  const AttnBwd attn("edge_attn_bn_bwd16", &g, qkvs, pifc, prpc, ea, alpha,
                     row_ptr, csr_src, col_ptr, csc_dst, csc_eid, heads);
  const int n = attn.s.n, h = attn.s.h;
  CHECK_IN(x); CHECK_IN(mask); CHECK_IN(gamma); CHECK_IN(mean);
  CHECK_IN(invstd);
  TORCH_CHECK(n > 0, "edge_attn_bn_bwd16 needs at least one node");
  TORCH_CHECK(h == 256 || h == 512, "edge_attn_bn_bwd16 covers H = 256, 512");
  TORCH_CHECK(qkvs.scalar_type() == torch::kBFloat16 &&
                  g.scalar_type() == torch::kBFloat16 &&
                  x.scalar_type() == torch::kBFloat16,
              "edge_attn_bn_bwd16 takes bf16 qkvs, g and x");
  TORCH_CHECK(x.dim() == 2 && x.size(0) == n && x.size(1) == h,
              "edge_attn_bn_bwd16: x must be [n, h]");
  TORCH_CHECK(mask.scalar_type() == torch::kUInt8,
              "edge_attn_bn_bwd16 needs the BN forward's keep mask");
  TORCH_CHECK(gamma.numel() == h && mean.numel() == h && invstd.numel() == h &&
                  gamma.scalar_type() == torch::kFloat32 &&
                  mean.scalar_type() == torch::kFloat32 &&
                  invstd.scalar_type() == torch::kFloat32,
              "gamma/mean/invstd must be fp32 [h]");
  const bool sync = partials_global_opt.has_value();
  TORCH_CHECK(sync == partials_local_opt.has_value(),
              "partials_global and partials_local come together");
  torch::Tensor partials_global, partials_local;
  if (sync) {
    partials_global = *partials_global_opt;
    partials_local = *partials_local_opt;
  }
  auto fopt = qkvs.options().dtype(torch::kFloat32);
  auto aff =
      bn_affine_out(dgamma_sink, dbeta_sink, qkvs, h, "edge_attn_bn_bwd16");
  AttnBnBwd bn{};
  bn.x = x.data_ptr();
  bn.mask = bn_mask_ptr(mask, x);
  bn.mean = mean.data_ptr<float>();
  bn.invstd = invstd.data_ptr<float>();
  bn.gamma = gamma.data_ptr<float>();
  bn.count = n;
  bn.keep_inv = (float)keep_inv;
  torch::Tensor partials, slab;  // alive until the launches are queued
  if (sync) {
    CHECK_IN(partials_global); CHECK_IN(partials_local);
    TORCH_CHECK(partials_global.numel() == 2 * h + 1 &&
                    partials_local.numel() >= 2 * h &&
                    partials_global.scalar_type() == torch::kFloat32 &&
                    partials_local.scalar_type() == torch::kFloat32,
                "edge_attn_bn_bwd16 expects fp32 [2h+1] partials with the "
                "global count in the tail slot");
    bn.partials = partials_global.data_ptr<float>();
    bn.count_ptr = partials_global.data_ptr<float>() + 2 * h;
    launch_bn_grad_affine(partials_local.data_ptr<float>(), aff.pg, aff.pb, h,
                          cur_stream(), aff.acc);
  } else {
    partials = torch::empty({2 * h}, fopt);
    slab = bn_wide_slab(x);
    launch_bn_bwd_partials_affine16(
        g.data_ptr(), x.data_ptr(), bn.mask, bn.mean, bn.invstd, n, h,
        partials.data_ptr<float>(), bn.keep_inv, bn_slab_ptr(slab), aff.pg,
        aff.pb, cur_stream(), aff.acc);
    bn.partials = partials.data_ptr<float>();
  }
  auto out = attn.run(&bn);
  return {out[0], out[1], aff.dgamma, aff.dbeta};
}

// Backward of edge_attention_fused (bf16 qkvs, fp32 output) whose only
// upstream gradient is the pattern pool's: gout [graphs, h] is the gradient
// of the pooled output and the kernels form g[i] = gout[batch[i]] * probs[i]
// / nn[i] themselves.  -> {dqkvs, de}, the bits of seg_pool_bwd followed by
// edge_attn_fused_bwd, without the [n, h] gradient in between.
std::vector<torch::Tensor> edge_attn_pool_bwd16(
    torch::Tensor gout, torch::Tensor probs, torch::Tensor nn,
    torch::Tensor batch, torch::Tensor qkvs, torch::Tensor pifc,
    torch::Tensor prpc, torch::Tensor ea, torch::Tensor alpha,
    torch::Tensor row_ptr, torch::Tensor csr_src, torch::Tensor col_ptr,
    torch::Tensor csc_dst, torch::Tensor csc_eid, int64_t heads = 1) {
  const AttnBwd attn("edge_attn_pool_bwd16", nullptr, qkvs, pifc, prpc, ea,
                     alpha, row_ptr, csr_src, col_ptr, csc_dst, csc_eid,
                     heads);
  const int n = attn.s.n, h = attn.s.h;
  CHECK_IN(gout); CHECK_IN(probs); CHECK_IN(nn); CHECK_IN(batch);
  TORCH_CHECK(h == 256 || h == 512, "edge_attn_pool_bwd16 covers H = 256, 512");
  TORCH_CHECK(gout.scalar_type() == torch::kFloat32 && gout.dim() == 2 &&
                  gout.size(1) == h,
              "gout must be fp32 [graphs, h]");
  TORCH_CHECK(probs.scalar_type() == torch::kFloat32 &&
                  nn.scalar_type() == torch::kFloat32 &&
                  batch.scalar_type() == torch::kInt64 &&
                  probs.numel() == n && nn.numel() == n && batch.numel() == n,
              "probs/nn (fp32) and batch (int64) must have one entry per node");
  AttnPoolBwd pool{};
  pool.gout = gout.data_ptr<float>();
  pool.probs = probs.data_ptr<float>();
  pool.nn = nn.data_ptr<float>();
  pool.batch = batch.data_ptr<long>();
  return attn.run(nullptr, &pool);
}

torch::Tensor seg_pool_fwd16(torch::Tensor x, torch::Tensor probs,
                             torch::Tensor nn, torch::Tensor batch_ptr,
                             int64_t num_graphs) {
  CHECK_IN(x); CHECK_IN(probs); CHECK_IN(nn); CHECK_IN(batch_ptr);
  const int h = x.size(1);
  const long p = seg_pool_parts(x.size(0), num_graphs);
  auto fopt = x.options().dtype(torch::kFloat32);
  auto partial = torch::empty({num_graphs * p, h}, fopt);
  auto out = torch::empty({num_graphs, h}, fopt);
  launch_seg_pool_fwd16(x.data_ptr(), probs.data_ptr<float>(),
                        nn.data_ptr<float>(), batch_ptr.data_ptr<int>(),
                        partial.data_ptr<float>(), out.data_ptr<float>(),
                        (int)num_graphs, (int)p, h, cur_stream());
  return out;
}

torch::Tensor seg_pool_bwd16(torch::Tensor gout, torch::Tensor probs,
                             torch::Tensor nn, torch::Tensor batch) {
  CHECK_IN(gout); CHECK_IN(batch);
  const long n = batch.size(0);
  const int h = gout.size(1);
  auto dx = torch::empty({n, h}, gout.options().dtype(torch::kBFloat16));
  launch_seg_pool_bwd16(gout.data_ptr<float>(), probs.data_ptr<float>(),
                        nn.data_ptr<float>(), batch.data_ptr<long>(),
                        dx.data_ptr(), n, h, cur_stream());
  return dx;
}

// Gate of the dgrad-as-glds-NT path (linear_dgrad16_o16), shared with the
// forward so that it can hand over the transposed weight image.
using gemm_dispatch::dgrad_glds_ok;

// -> (y, wt16): y = x . w^T + b in bf16.  With want_wt, and where the dgrad
// gate will accept the shape, wt16 is the transposed bf16 weight image
// [k, n] that the dgrad consumes, written by the same launch that makes the
// forward's own [n, k] image; otherwise it is an empty tensor.
static std::vector<torch::Tensor> linear_fwd_a16o16_impl(torch::Tensor x,
                                                         torch::Tensor w,
                                                         torch::Tensor b,
                                                         bool fp16c,
                                                         bool want_wt,
                                                         int64_t variant = 0,
                                                         OptTensor out =
                                                             std::nullopt) {
  namespace gd = gemm_dispatch;
  const auto [m, n, k] =
      linear_gate(want_wt ? "linear_fwd_a16o16_wt" : "linear_fwd_a16o16",
                  LIN_FWD, x, torch::kBFloat16, w, torch::kFloat32, &b);
  // variant != 0 forces the streaming (1) or the A-resident (2) glds kernel
  // for any shape that kernel can run; out, if given, receives y in its
  // first m rows (a test hook: the rows behind them must stay untouched)
  TORCH_CHECK(variant == gd::FWD_AUTO ||
                  (!fp16c && variant == gd::FWD_STREAM &&
                   gd::fwd_stream_can(m, n, k)) ||
                  (!fp16c && variant == gd::FWD_RESIDENT &&
                   gd::fwd_resident_can(m, n, k)),
              "linear_fwd_a16o16: variant ", variant, " cannot run [", m, ", ",
              k, "] x [", n, ", ", k, "]^T (1 needs bf16 compute, n % 128 == "
              "0 and k % 32 == 0; 2 needs bf16 compute, n % 128 == 0 and k == "
              "256)");
  torch::Tensor y;
  if (out.has_value() && out->defined()) {
    CHECK_IN((*out));
    TORCH_CHECK(out->scalar_type() == torch::kBFloat16 && out->dim() == 2 &&
                    out->size(0) >= m && out->size(1) == n,
                "out must be bf16 [>= m, n]");
    y = out->narrow(0, 0, m);
  } else {
    y = torch::empty({m, n}, x.options());  // bf16
  }
  auto wt16 = torch::empty({0}, x.options());
  if (m == 0) return {y, wt16};  // no rows: nothing to launch
  const float* bias = bias_ptr(b);
  if (fp16c) {
    launch_gemm_fp16_nt_a16o16(x.data_ptr(), w.data_ptr<float>(), bias,
                               y.data_ptr(), m, n, k, cur_stream());
    return {y, wt16};
  }
  // glds fast path (direct-to-LDS staging): needs 16-B-aligned rows, full
  // BK tiles in k, and n a multiple of the 128-wide tile.  The bf16 weight
  // copy costs one trivial convert kernel per call (n*k elements).
  const int fv = variant != gd::FWD_AUTO ? (int)variant
                                         : fwd_variant_for(m, n, k);
  if (fv != 0) {
    auto w16 = torch::empty({n, k}, x.options());  // bf16
    if (want_wt && dgrad_glds_ok(m, n, k)) {
      wt16 = torch::empty({k, n}, x.options());  // bf16, transposed
      launch_convert_w16_both(w.data_ptr<float>(), w16.data_ptr(),
                              wt16.data_ptr(), n, k, cur_stream());
    } else {
      launch_convert_w16(w.data_ptr<float>(), w16.data_ptr(), (long)n * k,
                         cur_stream());
    }
    if (fv == gd::FWD_RESIDENT)
      launch_gemm_a16_resident_nt(x.data_ptr(), w16.data_ptr(), bias,
                                  y.data_ptr(), m, n, k, cur_stream());
    else
      launch_gemm_a16_glds_nt(x.data_ptr(), w16.data_ptr(), bias,
                              y.data_ptr(), /*c16=*/1, m, n, k, false,
                              cur_stream());
    return {y, wt16};
  }
  launch_gemm_bf16_nt_a16o16(x.data_ptr(), w.data_ptr<float>(), bias,
                             y.data_ptr(), m, n, k, cur_stream());
  return {y, wt16};
}

// -> (w16 [n, k], wt16 [k, n]): the two bf16 weight images on their own
std::vector<torch::Tensor> convert_w16_both(torch::Tensor w) {
  CHECK_IN(w);
  TORCH_CHECK(w.scalar_type() == torch::kFloat32 && w.dim() == 2,
              "w must be fp32 [n, k]");
  const int n = w.size(0);
  const int k = w.size(1);
  auto opt = w.options().dtype(torch::kBFloat16);
  auto w16 = torch::empty({n, k}, opt);
  auto wt16 = torch::empty({k, n}, opt);
  launch_convert_w16_both(w.data_ptr<float>(), w16.data_ptr(),
                          wt16.data_ptr(), n, k, cur_stream());
  return {w16, wt16};
}

torch::Tensor linear_fwd_a16o16(torch::Tensor x, torch::Tensor w,
                                torch::Tensor b, bool fp16c = false,
                                int64_t variant = 0,
                                OptTensor out = std::nullopt) {
  return linear_fwd_a16o16_impl(x, w, b, fp16c, false, variant, out)[0];
}

std::vector<torch::Tensor> linear_fwd_a16o16_wt(torch::Tensor x,
                                                torch::Tensor w,
                                                torch::Tensor b,
                                                bool fp16c = false) {
  return linear_fwd_a16o16_impl(x, w, b, fp16c, true);
}

torch::Tensor linear_dgrad16_o16(torch::Tensor g, torch::Tensor w,
                                 bool fp16c = false,
                                 c10::optional<torch::Tensor> wt16_in =
                                     c10::nullopt) {
  const auto [m, n, k] = linear_gate("linear_dgrad16_o16", LIN_DGRAD, g,
                                     torch::kBFloat16, w, torch::kFloat32);
  auto dx = torch::empty({m, k}, g.options());  // bf16
  if (m == 0) return dx;  // no rows: nothing to launch
  if (fp16c) {
    launch_gemm_fp16_nn_a16o16(g.data_ptr(), w.data_ptr<float>(),
                               dx.data_ptr(), m, n, k, cur_stream());
    return dx;
  }
  // dgrad as glds-NT: dx[M,k] = g[M,n] . (w^T)[k,n]^T — a transposed bf16
  // copy of the weight turns the NN contraction into the NT fast path.  The
  // forward hands the copy over (wt16_in) where it made one; otherwise it
  // is converted here.
  if (dgrad_glds_ok(m, n, k)) {
    torch::Tensor wt16;
    if (wt16_in.has_value() && wt16_in->defined() && wt16_in->numel() > 0) {
      wt16 = *wt16_in;
      CHECK_IN(wt16);
      TORCH_CHECK(wt16.scalar_type() == torch::kBFloat16 && wt16.dim() == 2 &&
                      wt16.size(0) == k && wt16.size(1) == n,
                  "wt16 must be the bf16 [k, n] image of w");
    } else {
      wt16 = torch::empty({k, n}, g.options());  // bf16, transposed
      launch_transpose_convert_w16(w.data_ptr<float>(), wt16.data_ptr(), n, k,
                                   cur_stream());
    }
    launch_gemm_a16_glds_nt(g.data_ptr(), wt16.data_ptr(), nullptr,
                            dx.data_ptr(), /*c16=*/1, m, k, n, false,
                            cur_stream());
    return dx;
  }
  launch_gemm_bf16_nn_a16o16(g.data_ptr(), w.data_ptr<float>(),
                             dx.data_ptr(), m, n, k, cur_stream());
  return dx;
}

std::vector<torch::Tensor> linear_wgrad16_b16(torch::Tensor g, torch::Tensor x,
                                              bool has_bias,
                                              bool fp16c = false,
                                              OptTensor dw_sink = std::nullopt,
                                              OptTensor db_sink = std::nullopt,
                                              int64_t tile = 0) {
  const auto [m, n, k] = linear_gate("linear_wgrad16_b16", LIN_WGRAD, g,
                                     torch::kBFloat16, x, torch::kBFloat16);
  // tile != 0 forces an output tile of the glds TN kernel (1 / 2 / 3 =
  // 128x128 / 256x128 / 256x256) for any shape that kernel supports
  const char* det = getenv("PERTGNN_DETERMINISTIC");
  const bool glds = gemm_dispatch::wgrad_glds_ok(m, n, k, det && det[0] == '1');
  TORCH_CHECK(tile == 0 ||
                  (glds && !fp16c && glds_tn_tile_for(m, n, k, (int)tile) > 0),
              "linear_wgrad16_b16: tile ", tile, " cannot run [", m, ", ", n,
              "]^T x [", m, ", ", k, "] (needs bf16 compute, m >= 512, n "
              "and k multiples of the tile, not deterministic)");
  auto fopt = x.options().dtype(torch::kFloat32);
  float* dw_ptr = grad_sink(dw_sink, x, {n, k}, "linear_wgrad16_b16");
  float* db_ptr = grad_sink(db_sink, x, {n}, "linear_wgrad16_b16");
  const bool acc = dw_ptr != nullptr;
  TORCH_CHECK((db_ptr != nullptr) == (acc && has_bias),
              "linear_wgrad16_b16: a db sink comes with a dw sink and a bias");
  torch::Tensor dw = torch::empty({0}, fopt), db = torch::empty({0}, fopt);
  if (m == 0) {  // no rows: the sums over them are zero, nothing to launch
    if (acc) return {dw, db};
    return {torch::zeros({n, k}, fopt), torch::zeros({has_bias ? n : 0}, fopt)};
  }
  if (!acc) {
    // dw and db are views of one buffer, so the glds path clears both with a
    // single memset (the other paths clear the two views on their own)
    const long nk = (long)n * k;
    auto buf = torch::empty({nk + (has_bias ? n : 0)}, fopt);
    dw = buf.narrow(0, 0, nk).view({n, k});
    dw_ptr = dw.data_ptr<float>();
    if (has_bias) {
      db = buf.narrow(0, nk, n);
      db_ptr = db.data_ptr<float>();
    }
  }
  if (fp16c) {
    launch_gemm_fp16_tn_a16b16(g.data_ptr(), x.data_ptr(), dw_ptr, db_ptr, m,
                               n, k, cur_stream(), acc);
    return {dw, db};
  }
  // glds TN fast path (panel-major images + ds_read_b64_tr_b16 fragments);
  // split-K atomics => not for the deterministic mode
  if (glds) {
    launch_gemm_a16_glds_tn(g.data_ptr(), x.data_ptr(), dw_ptr, db_ptr, m, n,
                            k, cur_stream(), acc, (int)tile);
    return {dw, db};
  }
  launch_gemm_bf16_tn_a16b16(g.data_ptr(), x.data_ptr(), dw_ptr, db_ptr, m, n,
                             k, cur_stream(), acc);
  return {dw, db};
}

// ---------------------------------------------------------------------------
// linear_path: which kernel a linear op takes, from the same predicates
// (hip/gemm_dispatch.h) that the bindings and launchers above decide by.
// Host arithmetic only: launches nothing and never touches the device.
//   op   "fwd" (y = x.w^T + b), "dgrad" (dx = g.w), "wgrad" (dw = g^T.x, db)
//   x [m, k], w [n, k]
//   io   "f32": linear_fwd / linear_dgrad / linear_wgrad (and gemm_*), fp32
//               in and out, prec 0 / 1 / 2 = fp32 / bf16 / fp16 compute
//        "o16": linear_fwd_bf16_o16 / linear_dgrad16 / linear_wgrad16 (fp32
//               x, bf16 y and g), prec 1
//        "a16": linear_fwd_a16o16 / linear_dgrad16_o16 / linear_wgrad16_b16
//               (bf16 x, y and g), prec 1, or 2 for fp16 compute
// Labels: glds_nt_128x128, glds_nt_128x256, glds_tn, skinny_nn, and
// {f32,reg}_{nt,nn,tn}_{64,128} (fp32 / register-staging MFMA kernels, tile
// edge), "_fp16" appended for fp16 compute, "/s=<split-K slices>" appended
// for wgrad; "none" for m == 0.  The experiment knobs (PERTGNN_GEMM_*,
// PERTGNN_GLDS_*) are taken at their defaults.
// ---------------------------------------------------------------------------
std::string linear_path(const std::string& op, int64_t m64, int64_t n64,
                        int64_t k64, const std::string& io, int64_t prec,
                        bool deterministic) {
  namespace gd = gemm_dispatch;
  TORCH_CHECK(m64 >= 0 && n64 > 0 && k64 > 0 && m64 <= INT_MAX &&
                  n64 <= INT_MAX && k64 <= INT_MAX,
              "linear_path: bad shape");
  const int m = (int)m64, n = (int)n64, k = (int)k64;
  const int iop = op == "fwd" ? 0 : op == "dgrad" ? 1 : op == "wgrad" ? 2 : -1;
  TORCH_CHECK(iop >= 0, "linear_path: op must be fwd, dgrad or wgrad");
  const bool f32io = io == "f32", o16 = io == "o16", a16 = io == "a16";
  TORCH_CHECK(f32io || o16 || a16, "linear_path: io must be f32, o16 or a16");
  TORCH_CHECK(f32io ? (prec >= 0 && prec <= 2)
                    : o16 ? prec == 1 : (prec == 1 || prec == 2),
              "linear_path: no binding with this io and prec");
  if (m == 0) return "none";  // the bindings return before launching
  const std::string fp16 = prec == 2 ? "_fp16" : "";
  const std::string fam = prec == 0 ? "f32" : "reg";
  const auto tile = [](bool big) { return big ? "128" : "64"; };
  if (iop == 0) {
    if (a16 && prec == 1 && gd::fwd_glds_ok(m, n, k))
      return gd::glds_nt_wide(m, n, k) ? "glds_nt_128x256" : "glds_nt_128x128";
    return fam + "_nt_" + tile(gd::tile128(m, n)) + fp16;
  }
  if (iop == 1) {
    if (a16 && prec == 1 && gd::dgrad_glds_ok(m, n, k))
      return gd::glds_nt_wide(m, k, n) ? "glds_nt_128x256" : "glds_nt_128x128";
    if (o16 && gd::dgrad_skinny(m)) return "skinny_nn";
    return fam + "_nn_" + tile(gd::tile128(m, k)) + fp16;
  }
  if (a16 && prec == 1 && gd::wgrad_glds_ok(m, n, k, deterministic))
    return "glds_tn/s=" +
           std::to_string(gd::glds_tn_slices(
               m, gd::glds_tn_tiles(gd::glds_tn_tile(m, n, k), n, k)));
  return fam + "_tn_" + tile(gd::tn_tile128(n, k)) + fp16 + "/s=" +
         std::to_string(gd::tn_slices(m, gd::tn_tiles(n, k),
                                      prec == 0 ? 32 : 64, deterministic));
}

// Output tile of the glds TN wgrad (linear_wgrad16_b16, bf16 compute) at a
// shape, as it runs in this process: "128x128", "256x128" or "256x256";
// "none" where the shape is not on that kernel.  Unlike linear_path it
// follows set_wgrad_tile.
std::string wgrad_tile(int64_t m, int64_t n, int64_t k, bool deterministic) {
  TORCH_CHECK(m >= 0 && n > 0 && k > 0 && m <= INT_MAX && n <= INT_MAX &&
                  k <= INT_MAX, "wgrad_tile: bad shape");
  if (!gemm_dispatch::wgrad_glds_ok((int)m, (int)n, (int)k, deterministic))
    return "none";
  return gemm_dispatch::tn_tile_name(
      glds_tn_tile_for((int)m, (int)n, (int)k, gemm_dispatch::TN_AUTO));
}

// Test hook: the tile every later glds TN wgrad of this process takes where
// its shape allows it (0: back to the dispatch's choice).
void set_wgrad_tile(int64_t tile) {
  TORCH_CHECK(tile >= 0 && tile <= gemm_dispatch::TN_256x256,
              "set_wgrad_tile: tile must be 0 (auto), 1, 2 or 3");
  set_glds_tn_tile((int)tile);
}

// Kernel of the glds forward (linear_fwd_a16o16, bf16 compute) at a shape, as
// it runs in this process: "stream" (every block stages its own A K-tiles),
// "resident" (a block keeps its A row tile in LDS and sweeps the column
// tiles), or "none" where the shape is not on the glds forward.  Both give
// the same bits and share linear_path's label; unlike linear_path this
// follows set_fwd_variant and PERTGNN_NO_FWD_RESIDENT.
std::string fwd_variant(int64_t m, int64_t n, int64_t k) {
  TORCH_CHECK(m >= 0 && n > 0 && k > 0 && m <= INT_MAX && n <= INT_MAX &&
                  k <= INT_MAX, "fwd_variant: bad shape");
  const int v = m == 0 ? 0 : fwd_variant_for((int)m, (int)n, (int)k);
  return v == gemm_dispatch::FWD_RESIDENT ? "resident"
         : v == gemm_dispatch::FWD_STREAM ? "stream" : "none";
}

// Test hook: the kernel every later glds forward of this process takes where
// the A-resident kernel can run the shape, rows below the glds gate included
// (0: back to the dispatch's choice).
void set_fwd_variant(int64_t variant) {
  TORCH_CHECK(variant >= 0 && variant <= gemm_dispatch::FWD_RESIDENT,
              "set_fwd_variant: variant must be 0 (auto), 1 (stream) or 2 "
              "(resident)");
  set_fwd_variant_hook((int)variant);
}

// Every label linear_path can return, as "io|prec|op|label"; the wgrad labels
// stand once with "/s=1" (plain stores) and once with "/s>1" (atomic split-K).
std::vector<std::string> linear_path_labels() {
  std::vector<std::string> out;
  const auto add = [&](const char* io, int prec, const char* op,
                       const std::string& label) {
    out.push_back(std::string(io) + "|" + std::to_string(prec) + "|" + op +
                  "|" + label);
  };
  const auto reg = [&](const char* io, int prec) {
    const std::string fam = prec == 0 ? "f32" : "reg";
    const std::string fp16 = prec == 2 ? "_fp16" : "";
    for (const char* t : {"64", "128"}) {
      add(io, prec, "fwd", fam + "_nt_" + t + fp16);
      add(io, prec, "dgrad", fam + "_nn_" + t + fp16);
      for (const char* s : {"/s=1", "/s>1"})
        add(io, prec, "wgrad", fam + "_tn_" + t + fp16 + s);
    }
  };
  for (int prec = 0; prec <= 2; ++prec) reg("f32", prec);
  reg("o16", 1);
  add("o16", 1, "dgrad", "skinny_nn");
  reg("a16", 1);
  reg("a16", 2);
  for (const char* op : {"fwd", "dgrad"})
    for (const char* l : {"glds_nt_128x128", "glds_nt_128x256"})
      add("a16", 1, op, l);
  for (const char* s : {"/s=1", "/s>1"})
    add("a16", 1, "wgrad", std::string("glds_tn") + s);
  return out;
}

// ---------------------------------------------------------------------------
// Grouped P tables: P = table @ we^T for both embedding tables and every
// layer in one launch; the backward in one dgrad launch (summed over layers
// into the two table gradients) and one wgrad launch.
// ---------------------------------------------------------------------------

namespace {

// shared operand checks; returns h
int ptables_check(const torch::Tensor& ifc_table,
                  const torch::Tensor& rpc_table,
                  const std::vector<torch::Tensor>& we_ifc,
                  const std::vector<torch::Tensor>& we_rpc) {
  CHECK_IN(ifc_table); CHECK_IN(rpc_table);
  TORCH_CHECK(ifc_table.dim() == 2 && rpc_table.dim() == 2,
              "ptables: tables must be 2-D");
  TORCH_CHECK(ifc_table.scalar_type() == torch::kFloat32 &&
                  rpc_table.scalar_type() == torch::kFloat32,
              "ptables: tables must be float32");
  const int64_t h = ifc_table.size(1);
  TORCH_CHECK(h > 0 && rpc_table.size(1) == h,
              "ptables: tables must share a non-empty hidden size");
  TORCH_CHECK(!we_ifc.empty() && we_ifc.size() == we_rpc.size(),
              "ptables: need one we_ifc and one we_rpc per layer, got ",
              we_ifc.size(), " and ", we_rpc.size());
  for (const auto* list : {&we_ifc, &we_rpc})
    for (const auto& w : *list) {
      TORCH_CHECK(w.is_cuda() && w.device() == ifc_table.device(),
                  "ptables: weight must be on the tables' GPU");
      TORCH_CHECK(w.is_contiguous(), "ptables: weight must be contiguous");
      TORCH_CHECK(w.scalar_type() == torch::kFloat32,
                  "ptables: weight must be float32");
      TORCH_CHECK(w.dim() == 2 && w.size(0) == h && w.size(1) == h,
                  "ptables: weight must be [", h, ", ", h, "]");
    }
  TORCH_CHECK(ifc_table.size(0) < (1 << 30) && rpc_table.size(0) < (1 << 30) &&
                  h < (1 << 15),
              "ptables: table too large");
  return (int)h;
}

}  // namespace

// -> [pifc_0 .. pifc_{L-1}, prpc_0 .. prpc_{L-1}], each bf16 and bit-equal to
// linear_fwd_bf16_o16(table, we_l)
std::vector<torch::Tensor> ptables_fwd(torch::Tensor ifc_table,
                                       torch::Tensor rpc_table,
                                       std::vector<torch::Tensor> we_ifc,
                                       std::vector<torch::Tensor> we_rpc) {
  const int h = ptables_check(ifc_table, rpc_table, we_ifc, we_rpc);
  const int layers = (int)we_ifc.size();
  auto opt = ifc_table.options().dtype(torch::kBFloat16);
  std::vector<torch::Tensor> out;
  std::vector<const float*> a, w;
  std::vector<void*> c;
  std::vector<int> m;
  for (int t = 0; t < 2; ++t) {
    const auto& table = t == 0 ? ifc_table : rpc_table;
    const auto& ws = t == 0 ? we_ifc : we_rpc;
    for (int l = 0; l < layers; ++l) {
      out.push_back(torch::empty({table.size(0), h}, opt));
      a.push_back(table.data_ptr<float>());
      w.push_back(ws[l].data_ptr<float>());
      c.push_back(out.back().data_ptr());
      m.push_back((int)table.size(0));
    }
  }
  launch_ptables_fwd(2 * layers, a.data(), w.data(), c.data(), m.data(), h, h,
                     cur_stream());
  return out;
}

// dP: 2L tensors in ptables_fwd's output order, an EMPTY tensor standing for
// a missing (zero) gradient.  Returns (d_ifc_table [V,h], d_rpc_table [R,h],
// dW [2L,h,h]) as views of one buffer, so one memset covers every atomic
// accumulation; dW[g] of a missing dP[g] is zero.  dgrad_splits > 1 splits
// the dgrad's layer sum over that many blocks (atomics; ignored under
// PERTGNN_DETERMINISTIC=1, like the wgrad's split-K).
// Gradient sinks: d_ifc_sink / d_rpc_sink for the two tables, dw_sinks empty
// (none) or 2L entries in dP's order, each a sink or None.  An output with a
// sink is added into it and left out of the buffer: its table slot of the
// result is an empty tensor, and dW holds only the groups WITHOUT a sink, in
// order.  The sink of a missing dP[g] is not touched; with every output sunk
// nothing is allocated or cleared.
std::vector<torch::Tensor> ptables_bwd(std::vector<torch::Tensor> dP,
                                       torch::Tensor ifc_table,
                                       torch::Tensor rpc_table,
                                       std::vector<torch::Tensor> we_ifc,
                                       std::vector<torch::Tensor> we_rpc,
                                       int64_t dgrad_splits,
                                       OptTensor d_ifc_sink = std::nullopt,
                                       OptTensor d_rpc_sink = std::nullopt,
                                       std::vector<OptTensor> dw_sinks = {}) {
  const int h = ptables_check(ifc_table, rpc_table, we_ifc, we_rpc);
  const int layers = (int)we_ifc.size();
  TORCH_CHECK((int)dP.size() == 2 * layers, "ptables_bwd: need ", 2 * layers,
              " dP entries, got ", dP.size());
  TORCH_CHECK(dw_sinks.empty() || (int)dw_sinks.size() == 2 * layers,
              "ptables_bwd: need no or ", 2 * layers, " dw_sinks entries, got ",
              dw_sinks.size());
  const int64_t rows[2] = {ifc_table.size(0), rpc_table.size(0)};
  float* const sink_t[2] = {
      grad_sink(d_ifc_sink, ifc_table, {rows[0], h}, "ptables_bwd"),
      grad_sink(d_rpc_sink, ifc_table, {rows[1], h}, "ptables_bwd")};
  std::vector<float*> sink_w(2 * layers, nullptr);
  int n_ret = 0;  // dW groups without a sink: the ones returned
  for (int g = 0; g < 2 * layers; ++g) {
    if (!dw_sinks.empty())
      sink_w[g] = grad_sink(dw_sinks[g], ifc_table, {h, h}, "ptables_bwd");
    if (!sink_w[g]) ++n_ret;
  }
  bool missing = false;
  for (int g = 0; g < 2 * layers; ++g) {
    const auto& d = dP[g];
    if (!d.defined() || d.numel() == 0) {
      missing |= rows[g / layers] > 0 && !sink_w[g];
      continue;
    }
    TORCH_CHECK(d.is_cuda() && d.device() == ifc_table.device(),
                "ptables_bwd: dP must be on the tables' GPU");
    TORCH_CHECK(d.is_contiguous(), "ptables_bwd: dP must be contiguous");
    TORCH_CHECK(d.scalar_type() == torch::kBFloat16,
                "ptables_bwd: dP must be bfloat16");
    TORCH_CHECK(d.dim() == 2 && d.size(0) == rows[g / layers] && d.size(1) == h,
                "ptables_bwd: dP[", g, "] must be [", rows[g / layers], ", ",
                h, "]");
  }
  const char* det_env = getenv("PERTGNN_DETERMINISTIC");
  const bool det = det_env && det_env[0] == '1';
  const int splits =
      det ? 1 : (int)std::min<int64_t>(std::max<int64_t>(dgrad_splits, 1), layers);

  const int64_t hh = (int64_t)h * h;
  const int64_t n_dw = n_ret * hh;
  const int64_t n_dt[2] = {sink_t[0] ? 0 : rows[0] * h,
                           sink_t[1] ? 0 : rows[1] * h};
  auto buf = torch::empty({n_dw + n_dt[0] + n_dt[1]}, ifc_table.options());
  auto none = torch::empty({0}, ifc_table.options());
  auto dW = buf.narrow(0, 0, n_dw).view({n_ret, h, h});
  auto d_ifc = sink_t[0] ? none
                         : buf.narrow(0, n_dw, n_dt[0]).view({rows[0], h});
  auto d_rpc = sink_t[1] ? none
                         : buf.narrow(0, n_dw + n_dt[0], n_dt[1])
                               .view({rows[1], h});

  std::vector<const void*> dp_w, dp_d;
  std::vector<const float*> a_w, w_d;
  std::vector<float*> dw_w;
  std::vector<int> m_w;
  std::unique_ptr<bool[]> sunk(new bool[2 * layers]);  // per launched group
  int npairs[2] = {0, 0};
  int ret = 0;  // index in dW of the next group without a sink
  for (int g = 0; g < 2 * layers; ++g) {
    const auto& d = dP[g];
    float* const dw_g =
        sink_w[g] ? sink_w[g] : buf.data_ptr<float>() + (ret++) * hh;
    if (!d.defined() || d.numel() == 0) continue;
    const int t = g / layers;
    const auto& table = t == 0 ? ifc_table : rpc_table;
    const auto& w = (t == 0 ? we_ifc : we_rpc)[g % layers];
    sunk[dp_w.size()] = sink_w[g] != nullptr;
    dp_w.push_back(d.data_ptr());
    a_w.push_back(table.data_ptr<float>());
    dw_w.push_back(dw_g);
    m_w.push_back((int)rows[t]);
    dp_d.push_back(d.data_ptr());
    w_d.push_back(w.data_ptr<float>());
    ++npairs[t];
  }
  auto s = cur_stream();
  // only what the buffer holds is ever cleared, never a sink
  const bool zero_dw =
      n_dw > 0 &&
      (missing ||
       launch_ptables_wgrad((int)dp_w.size(), dp_w.data(), a_w.data(),
                            dw_w.data(), m_w.data(), h, true, s, sunk.get()));
  const bool zero_dt = splits > 1 && n_dt[0] + n_dt[1] > 0;
  if (zero_dw || zero_dt) {
    float* beg = buf.data_ptr<float>() + (zero_dw ? 0 : n_dw);
    const int64_t cnt =
        (zero_dw ? n_dw : 0) + (zero_dt ? n_dt[0] + n_dt[1] : 0);
    const hipError_t err = hipMemsetAsync(beg, 0, cnt * sizeof(float), s);
    TORCH_CHECK(err == hipSuccess, "ptables_bwd: memset failed: ",
                hipGetErrorString(err));
  }
  float* outs[2] = {sink_t[0] ? sink_t[0] : d_ifc.data_ptr<float>(),
                    sink_t[1] ? sink_t[1] : d_rpc.data_ptr<float>()};
  const int ms[2] = {(int)rows[0], (int)rows[1]};
  // splits > 1 has cleared every table output that is not a sink
  const bool addto[2] = {sink_t[0] != nullptr || splits > 1,
                         sink_t[1] != nullptr || splits > 1};
  launch_ptables_dgrad(dp_d.data(), w_d.data(), npairs, outs, ms, h, splits,
                       addto, s);
  launch_ptables_wgrad((int)dp_w.size(), dp_w.data(), a_w.data(), dw_w.data(),
                       m_w.data(), h, false, s, sunk.get());
  return {d_ifc, d_rpc, dW};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  mod.def("ptables_fwd", &ptables_fwd, py::arg("ifc_table"),
          py::arg("rpc_table"), py::arg("we_ifc"), py::arg("we_rpc"));
  mod.def("ptables_bwd", &ptables_bwd, py::arg("dP"), py::arg("ifc_table"),
          py::arg("rpc_table"), py::arg("we_ifc"), py::arg("we_rpc"),
          py::arg("dgrad_splits") = 1, py::arg("d_ifc_sink") = py::none(),
          py::arg("d_rpc_sink") = py::none(),
          py::arg("dw_sinks") = std::vector<OptTensor>());
  mod.def("ptables_max_groups", &ptables_max_groups);
  mod.def("linear_fwd_bf16_o16", &linear_fwd_bf16_o16);
  mod.def("linear_dgrad16", &linear_dgrad16);
  mod.def("linear_wgrad16", &linear_wgrad16, py::arg("g"), py::arg("x"),
          py::arg("has_bias"), py::arg("dw_sink") = py::none(),
          py::arg("db_sink") = py::none(), py::arg("tile") = 0);
  mod.def("vocab_scatter_dual", &vocab_scatter_dual);
  mod.def("linear_dgrad", &linear_dgrad);
  mod.def("linear_wgrad", &linear_wgrad);
  mod.def("embed_grouped_scatter_bal", &embed_grouped_scatter_bal);
  mod.def("edge_table_grad", &edge_table_grad, py::arg("de"), py::arg("idx1"),
          py::arg("lptr1"), py::arg("idx2"), py::arg("lptr2"),
          py::arg("idx3"), py::arg("lptr3"), py::arg("V"), py::arg("R"),
          py::arg("out_dtype"), py::arg("unroll") = 8);
  mod.def("embed_dgrad_fold", &embed_dgrad_fold, py::arg("dqkvs"),
          py::arg("idx1"), py::arg("lptr1"), py::arg("idx2"), py::arg("lptr2"),
          py::arg("idx3"), py::arg("lptr3"), py::arg("w4"), py::arg("f"),
          py::arg("h"), py::arg("rows"), py::arg("sink") = py::none(),
          py::arg("unroll") = 8, py::arg("seg_cols") = 256);
  mod.def("bn_stats", &bn_stats);
  // each BN operation under its fp32 name and its bf16 ("16") name
  const auto def_bn_fwd = [&mod](const char* name, auto fn) {
    mod.def(name, fn, py::arg("x"), py::arg("gamma"), py::arg("beta"),
            py::arg("running_mean"), py::arg("running_var"),
            py::arg("momentum"), py::arg("eps"), py::arg("training"),
            py::arg("relu"), py::arg("dropout_p") = 0.0,
            py::arg("seed") = torch::Tensor());
  };
  def_bn_fwd("bn_relu_fwd", &bn_relu_fwd<false>);
  def_bn_fwd("bn_relu_fwd16", &bn_relu_fwd<true>);
  const auto def_bn_bwd = [&mod](const char* name, auto fn) {
    mod.def(name, fn, py::arg("g"), py::arg("x"), py::arg("gamma"),
            py::arg("mean"), py::arg("invstd"), py::arg("y"), py::arg("relu"),
            py::arg("keep_inv") = 1.0, py::arg("dgamma_sink") = py::none(),
            py::arg("dbeta_sink") = py::none());
  };
  def_bn_bwd("bn_relu_bwd", &bn_relu_bwd<false>);
  def_bn_bwd("bn_relu_bwd16", &bn_relu_bwd<true>);
  const auto def_bn_finalize = [&mod](const char* name, auto fn) {
    mod.def(name, fn, py::arg("x"), py::arg("partials"), py::arg("gamma"),
            py::arg("beta"), py::arg("running_mean"), py::arg("running_var"),
            py::arg("momentum"), py::arg("eps"), py::arg("training"),
            py::arg("relu"), py::arg("dropout_p") = 0.0,
            py::arg("seed") = torch::Tensor());
  };
  def_bn_finalize("bn_finalize_apply", &bn_finalize_apply<false>);
  def_bn_finalize("bn_finalize_apply16", &bn_finalize_apply<true>);
  const auto def_bn_partials = [&mod](const char* name, auto fn) {
    mod.def(name, fn, py::arg("g"), py::arg("x"), py::arg("y"),
            py::arg("mean"), py::arg("invstd"), py::arg("relu"),
            py::arg("keep_inv") = 1.0);
  };
  def_bn_partials("bn_bwd_partials", &bn_bwd_partials<false>);
  def_bn_partials("bn_bwd_partials16", &bn_bwd_partials<true>);
  const auto def_bn_apply = [&mod](const char* name, auto fn) {
    mod.def(name, fn, py::arg("g"), py::arg("x"), py::arg("y"),
            py::arg("mean"), py::arg("invstd"), py::arg("gamma"),
            py::arg("partials_global"), py::arg("partials_local"),
            py::arg("relu"), py::arg("keep_inv") = 1.0,
            py::arg("dgamma_sink") = py::none(),
            py::arg("dbeta_sink") = py::none());
  };
  def_bn_apply("bn_bwd_apply", &bn_bwd_apply<false>);
  def_bn_apply("bn_bwd_apply16", &bn_bwd_apply<true>);
  mod.def("vocab_scatter", &vocab_scatter);
  mod.def("collate_native", &collate_native,
          py::call_guard<py::gil_scoped_release>());
  mod.def("edge_attn_fused_fwd", &edge_attn_fused_fwd, py::arg("qkvs"),
          py::arg("pifc"), py::arg("prpc"), py::arg("edge_attr"),
          py::arg("row_ptr"), py::arg("csr_src"), py::arg("out16"),
          py::arg("heads") = 1);
  mod.def("edge_attn_fused_bwd", &edge_attn_fused_bwd, py::arg("g"),
          py::arg("qkvs"), py::arg("pifc"), py::arg("prpc"),
          py::arg("edge_attr"), py::arg("alpha"), py::arg("row_ptr"),
          py::arg("csr_src"), py::arg("col_ptr"), py::arg("csc_dst"),
          py::arg("csc_eid"), py::arg("heads") = 1);
  mod.def("edge_attn_fused_infer", &edge_attn_fused_infer, py::arg("qkvs"),
          py::arg("pifc"), py::arg("prpc"), py::arg("edge_attr"),
          py::arg("row_ptr"), py::arg("csr_src"), py::arg("bn_scale"),
          py::arg("bn_shift"), py::arg("relu"), py::arg("out16"),
          py::arg("heads") = 1);
  mod.def("embed_grouped_scatter", &embed_grouped_scatter);
  mod.def("linear_fwd", &linear_fwd);
  mod.def("linear_fwd_bf16", &linear_fwd_bf16);
  mod.def("linear_fwd_fp16", &linear_fwd_fp16);
  mod.def("linear_bwd_fp16", &linear_bwd_fp16);
  mod.def("linear_bwd_bf16", &linear_bwd_bf16);
  mod.def("gemm_nt_bf16", &gemm_nt_bf16);
  mod.def("gemm_nn_bf16", &gemm_nn_bf16);
  mod.def("gemm_tn_bf16", &gemm_tn_bf16);
  mod.def("linear_bwd", &linear_bwd);
  mod.def("gemm_nt", &gemm_nt);
  mod.def("gemm_nn", &gemm_nn);
  mod.def("gemm_tn", &gemm_tn);
  mod.def("edge_attn_fwd", &edge_attn_fwd);
  mod.def("edge_attn_bwd", &edge_attn_bwd);
  mod.def("seg_pool_fwd", &seg_pool_fwd);
  mod.def("seg_pool_bwd", &seg_pool_bwd);
  mod.def("embed_node_fwd", &embed_node_fwd, py::arg("x_raw"), py::arg("idx"), py::arg("table"), py::arg("out16") = false, py::arg("pad_to") = 0);
  mod.def("embed_edge_fwd", &embed_edge_fwd);
  mod.def("gather_rows", &gather_rows);
  mod.def("edge_attn_bn_bwd16", &edge_attn_bn_bwd16, py::arg("g"),
          py::arg("x"), py::arg("mask"), py::arg("gamma"), py::arg("mean"),
          py::arg("invstd"), py::arg("keep_inv"), py::arg("qkvs"),
          py::arg("pifc"), py::arg("prpc"), py::arg("edge_attr"),
          py::arg("alpha"), py::arg("row_ptr"), py::arg("csr_src"),
          py::arg("col_ptr"), py::arg("csc_dst"), py::arg("csc_eid"),
          py::arg("heads") = 1, py::arg("partials_global") = py::none(),
          py::arg("partials_local") = py::none(),
          py::arg("dgamma_sink") = py::none(),
          py::arg("dbeta_sink") = py::none());
  mod.def("edge_attn_pool_bwd16", &edge_attn_pool_bwd16, py::arg("gout"),
          py::arg("probs"), py::arg("nn"), py::arg("batch"), py::arg("qkvs"),
          py::arg("pifc"), py::arg("prpc"), py::arg("edge_attr"),
          py::arg("alpha"), py::arg("row_ptr"), py::arg("csr_src"),
          py::arg("col_ptr"), py::arg("csc_dst"), py::arg("csc_eid"),
          py::arg("heads") = 1);
  mod.def("seg_pool_fwd16", &seg_pool_fwd16);
  mod.def("seg_pool_bwd16", &seg_pool_bwd16);
  mod.def("linear_fwd_a16o16", &linear_fwd_a16o16, py::arg("x"), py::arg("w"),
          py::arg("b"), py::arg("fp16c") = false, py::arg("variant") = 0,
          py::arg("out") = py::none());
  mod.def("fwd_variant", &fwd_variant, py::arg("m"), py::arg("n"),
          py::arg("k"));
  mod.def("set_fwd_variant", &set_fwd_variant, py::arg("variant"));
  mod.def("convert_w16_both", &convert_w16_both, py::arg("w"));
  mod.def("linear_fwd_a16o16_wt", &linear_fwd_a16o16_wt, py::arg("x"),
          py::arg("w"), py::arg("b"), py::arg("fp16c") = false);
  mod.def("linear_dgrad16_o16", &linear_dgrad16_o16, py::arg("g"),
          py::arg("w"), py::arg("fp16c") = false,
          py::arg("wt16") = py::none());
  mod.def("linear_wgrad16_b16", &linear_wgrad16_b16, py::arg("g"),
          py::arg("x"), py::arg("has_bias"), py::arg("fp16c") = false,
          py::arg("dw_sink") = py::none(), py::arg("db_sink") = py::none(),
          py::arg("tile") = 0);
  mod.def("wgrad_tile", &wgrad_tile, py::arg("m"), py::arg("n"), py::arg("k"),
          py::arg("deterministic") = false);
  mod.def("set_wgrad_tile", &set_wgrad_tile, py::arg("tile"));
  mod.def("linear_path", &linear_path, py::arg("op"), py::arg("m"),
          py::arg("n"), py::arg("k"), py::arg("io"), py::arg("prec"),
          py::arg("deterministic") = false);
  mod.def("linear_path_labels", &linear_path_labels);
  mod.def("quantile_loss_fwd", &quantile_loss_fwd);
  mod.def("quantile_loss_bwd", &quantile_loss_bwd);
  mod.def("eval_metrics", &eval_metrics);
  mod.def("adam_step_dynamic", &adam_step_dynamic);
  mod.def("adam_step", &adam_step, py::arg("p"), py::arg("g"), py::arg("m"),
          py::arg("v"), py::arg("state"), py::arg("lr"), py::arg("b1"),
          py::arg("b2"), py::arg("eps"), py::arg("gscale") = 1.0);
  mod.def("adam_step_ex", &adam_step_ex, py::arg("p"), py::arg("g"),
          py::arg("m"), py::arg("v"), py::arg("state"), py::arg("sstate"),
          py::arg("hstate"), py::arg("slab"), py::arg("decay_mask"),
          py::arg("lr_table"), py::arg("lr"), py::arg("b1"), py::arg("b2"),
          py::arg("eps"), py::arg("gscale"), py::arg("wd"),
          py::arg("max_norm"), py::arg("backoff"), py::arg("growth"),
          py::arg("interval"));
}
