// bindings.cpp — pybind module for the gfx950 kernel library.
#include <torch/extension.h>

// elementwise.hip
void multi_tensor_unscale(std::vector<at::Tensor> grads, at::Tensor found_inf,
                          double inv_scale,
                          c10::optional<at::Tensor> partials);
void multi_tensor_sqsum(std::vector<at::Tensor> tensors, at::Tensor partials);
void norm_finalize(at::Tensor partials, long n, double max_norm,
                   c10::optional<at::Tensor> found_inf, at::Tensor out,
                   c10::optional<at::Tensor> stats);
void multi_tensor_scale(std::vector<at::Tensor> tensors, at::Tensor coef,
                        c10::optional<at::Tensor> found_inf);
long mt_chunk_elems();
void fused_sgd(std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
               std::vector<at::Tensor> bufs, double lr, double momentum,
               double wd, double nesterov, c10::optional<at::Tensor> found_inf,
               c10::optional<at::Tensor> grad_scale);
void fused_lars(std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
                std::vector<at::Tensor> bufs, at::Tensor partials,
                at::Tensor ratios, double lr, double momentum, double wd,
                double nesterov, double eta, double eps, bool trust_clip,
                c10::optional<at::Tensor> found_inf,
                c10::optional<at::Tensor> grad_scale);
void fused_adamw(std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
                 std::vector<at::Tensor> exp_avgs,
                 std::vector<at::Tensor> exp_avg_sqs, at::Tensor steps,
                 at::Tensor coefs, double lr, double beta1, double beta2,
                 double eps, double wd, bool decoupled,
                 c10::optional<at::Tensor> found_inf,
                 c10::optional<at::Tensor> grad_scale);
void fused_lamb(std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
                std::vector<at::Tensor> exp_avgs,
                std::vector<at::Tensor> exp_avg_sqs, at::Tensor steps,
                at::Tensor coefs, at::Tensor partials, at::Tensor ratios,
                double lr, double beta1, double beta2, double eps, double wd,
                bool trust_clip, double max_trust,
                c10::optional<at::Tensor> found_inf,
                c10::optional<at::Tensor> grad_scale);
long adam_ncoef();
void fused_lookahead(std::vector<at::Tensor> fast, std::vector<at::Tensor> slow,
                     double alpha, c10::optional<at::Tensor> found_inf);
at::Tensor cast_to_bf16(at::Tensor x);
at::Tensor pad8_channels(at::Tensor x);
at::Tensor nhwc_flatten(at::Tensor x);
at::Tensor nhwc_unflatten(at::Tensor dy, long C, long H, long W);
std::vector<at::Tensor> pack_conv_weight(at::Tensor w, bool pad8,
                                         bool want_wt2);
at::Tensor dropout_fwd(at::Tensor x, long thr, double scale, long call_seed);
at::Tensor dropout_bwd(at::Tensor dy, long thr, double scale, long call_seed);
at::Tensor relu_dropout_fwd(at::Tensor x, long thr, double scale,
                            long call_seed);

// ce.hip
std::vector<at::Tensor> ce_fwd(at::Tensor logits, at::Tensor target);
at::Tensor ce_bwd(at::Tensor logits, at::Tensor target, at::Tensor lse,
                  at::Tensor dloss);
at::Tensor argmax_correct(at::Tensor logits, at::Tensor target);
std::vector<at::Tensor> ce_mix_fwd(at::Tensor logits, at::Tensor target_a,
                                   at::Tensor target_b, at::Tensor lam,
                                   double smoothing);
at::Tensor ce_mix_bwd(at::Tensor logits, at::Tensor target_a,
                      at::Tensor target_b, at::Tensor lam, at::Tensor lse,
                      at::Tensor dloss, double smoothing);

// pool.hip
std::vector<at::Tensor> maxpool2x2_fwd(at::Tensor x);
at::Tensor maxpool2x2_bwd(at::Tensor dy, at::Tensor idx, long H, long W);
std::vector<at::Tensor> maxpool_fwd(at::Tensor x, long ks, long st, long pad);
at::Tensor maxpool_bwd(at::Tensor dy, at::Tensor idx, long H, long W,
                       long ks, long st, long pad);
at::Tensor global_avgpool_fwd(at::Tensor x);
at::Tensor global_avgpool_bwd(at::Tensor dy, long H, long W);

// bn.hip
std::vector<at::Tensor> bn_fwd_train(at::Tensor x, at::Tensor gamma,
                                     at::Tensor beta, at::Tensor running_mean,
                                     at::Tensor running_var, double momentum,
                                     double eps, bool fuse_relu,
                                     c10::optional<at::Tensor> residual,
                                     c10::optional<at::Tensor> pre_stats);
at::Tensor bn_fwd_eval(at::Tensor x, at::Tensor gamma, at::Tensor beta,
                       at::Tensor running_mean, at::Tensor running_var,
                       double eps, bool fuse_relu,
                       c10::optional<at::Tensor> residual);
std::vector<at::Tensor> bn_fwd_eval_mask(at::Tensor x, at::Tensor gamma,
                                         at::Tensor beta,
                                         at::Tensor running_mean,
                                         at::Tensor running_var, double eps,
                                         bool fuse_relu,
                                         c10::optional<at::Tensor> residual);
std::vector<at::Tensor> bn_bwd(at::Tensor x, at::Tensor dy, at::Tensor gamma,
                               at::Tensor save_mean, at::Tensor save_invstd,
                               at::Tensor mask, bool fuse_relu,
                               bool want_dresid,
                               c10::optional<at::Tensor> pre_slab,
                               bool eval_stats);
std::vector<at::Tensor> bn_fwd_train_pool2(at::Tensor x, at::Tensor gamma,
                                           at::Tensor beta,
                                           at::Tensor running_mean,
                                           at::Tensor running_var,
                                           double momentum, double eps,
                                           c10::optional<at::Tensor> pre_stats);
std::vector<at::Tensor> bn_bwd_pool2(at::Tensor x, at::Tensor dy_pooled,
                                     at::Tensor gamma, at::Tensor save_mean,
                                     at::Tensor save_invstd, at::Tensor code);
at::Tensor bn_sync_local(at::Tensor x, c10::optional<at::Tensor> pre_stats);
std::vector<at::Tensor> bn_sync_fwd(at::Tensor x, at::Tensor gathered,
                                    at::Tensor gamma, at::Tensor beta,
                                    at::Tensor running_mean,
                                    at::Tensor running_var, double momentum,
                                    double eps, bool fuse_relu,
                                    c10::optional<at::Tensor> residual);
at::Tensor bn_sync_bwd_local(at::Tensor x, at::Tensor dy,
                             at::Tensor save_mean, at::Tensor save_invstd,
                             at::Tensor mask, bool fuse_relu);
std::vector<at::Tensor> bn_sync_bwd_dx(at::Tensor x, at::Tensor dy,
                                       at::Tensor gamma, at::Tensor save_mean,
                                       at::Tensor save_invstd, at::Tensor mask,
                                       bool fuse_relu, at::Tensor gathered,
                                       at::Tensor count, bool want_dresid);

// gemm.hip
at::Tensor gemm_tn(at::Tensor A, at::Tensor B, c10::optional<at::Tensor> bias,
                   bool out_f32, long impl);
at::Tensor transpose_bf16(at::Tensor x);
at::Tensor col_sum(at::Tensor x);
at::Tensor linear_fwd(at::Tensor x, at::Tensor w, c10::optional<at::Tensor> bias,
                      long impl);
at::Tensor linear_dgrad(at::Tensor dy, at::Tensor w, long impl);
at::Tensor linear_wgrad(at::Tensor dy, at::Tensor x, long impl);
at::Tensor linear_act_fwd(at::Tensor x, at::Tensor w,
                          c10::optional<at::Tensor> bias, long thr,
                          double scale, long call_seed, long impl);
std::string linear_plan(long op, long M, long N, long K, long impl);
at::Tensor relu_drop_bwd(at::Tensor dy, at::Tensor y, double scale);

// conv.hip
at::Tensor conv2d_fwd(at::Tensor x, at::Tensor w, c10::optional<at::Tensor> bias,
                      long stride, long pad, long kwalk);
std::vector<at::Tensor> conv2d_fwd_stats(at::Tensor x, at::Tensor w,
                                         c10::optional<at::Tensor> bias,
                                         long stride, long pad, long kwalk);
at::Tensor conv2d_dgrad(at::Tensor dy, at::Tensor wt2, long N, long C, long H,
                        long W, long R, long S, long stride, long pad,
                        c10::optional<at::Tensor> addend, long group,
                        long kwalk);
std::tuple<at::Tensor, at::Tensor> conv2d_stem_fwd(
    at::Tensor x, at::Tensor w, c10::optional<at::Tensor> bias, long stride,
    long pad, bool want_stats, long stem);
std::string conv2d_stem_plan(long N, long C, long H, long W, long Ko, long R,
                             long S, long stride, long pad, long stem);
std::string conv2d_kloop_plan(long mode, long N, long C, long H, long W,
                              long Ko, long R, long S, long stride, long pad,
                              long kwalk);
std::tuple<std::string, long, long, long> conv2d_dgrad_plan(
    long N, long C, long H, long W, long Ko, long R, long S, long stride,
    long pad, long group);
std::vector<at::Tensor> conv2d_dgrad_bn(at::Tensor dy, at::Tensor wt2,
                                        long N, long C, long H, long W,
                                        long R, long S, long pad,
                                        at::Tensor bn_x, at::Tensor bn_mask,
                                        at::Tensor bn_mean,
                                        at::Tensor bn_invstd);
at::Tensor conv2d_wgrad(at::Tensor dy, at::Tensor x, long R, long S,
                        long stride, long pad, long walk);
std::vector<at::Tensor> conv2d_wgrad_bias(at::Tensor dy, at::Tensor x,
                                          long R, long S, long stride,
                                          long pad, long walk);
std::tuple<std::string, long, long, long> conv2d_wgrad_kloop_plan(
    long N, long C, long H, long W, long Ko, long R, long S, long stride,
    long pad, bool want_bias, long walk);
std::vector<std::tuple<long, long, long, bool>> conv2d_wgrad_walk_rows(
    long N, long C, long H, long W, long Ko, long R, long S, long stride,
    long pad, bool want_bias, long split, long chunk_row, long tiles);
std::tuple<std::string, long, bool> conv2d_wgrad_plan(
    long N, long C, long H, long W, long Ko, long R, long S, long stride,
    long pad, bool want_bias);

// dwconv.hip
std::tuple<at::Tensor, at::Tensor> dwconv2d_fwd(
    at::Tensor x, at::Tensor w, c10::optional<at::Tensor> bias, long stride,
    long pad, bool want_stats, long tr);
at::Tensor dwconv2d_dgrad(at::Tensor dy, at::Tensor w, long H, long W,
                          long stride, long pad, long tr);
std::tuple<at::Tensor, at::Tensor> dwconv2d_wgrad(at::Tensor dy, at::Tensor x,
                                                  long stride, long pad,
                                                  bool want_db, long tr);
std::tuple<long, long, long, long> dwconv2d_plan(std::string op, long N,
                                                 long C, long H, long W,
                                                 long stride, long pad,
                                                 long tr);

// dwconvk.hip
std::tuple<at::Tensor, at::Tensor> dwconvk2d_fwd(
    at::Tensor x, at::Tensor w, c10::optional<at::Tensor> bias, long stride,
    long pad, bool want_stats, long to);
at::Tensor dwconvk2d_dgrad(at::Tensor dy, at::Tensor w, long H, long W,
                           long stride, long pad, long to);
std::tuple<at::Tensor, at::Tensor> dwconvk2d_wgrad(at::Tensor dy, at::Tensor x,
                                                   long K, long stride,
                                                   long pad, bool want_db,
                                                   long to);
std::tuple<long, long, long, long> dwconvk2d_plan(std::string op, long N,
                                                  long C, long H, long W,
                                                  long K, long stride,
                                                  long pad, long to);

// gconv.hip
std::tuple<at::Tensor, at::Tensor> gconv2d_pack(at::Tensor w);
std::tuple<at::Tensor, at::Tensor> gconv2d_fwd(
    at::Tensor x, at::Tensor wimg, c10::optional<at::Tensor> bias, long groups,
    long stride, long pad, bool want_stats);
at::Tensor gconv2d_dgrad(at::Tensor dy, at::Tensor wimg_t, long H, long W,
                         long groups, long stride, long pad);
at::Tensor gconv2d_wgrad(at::Tensor dy, at::Tensor x, long groups, long stride,
                         long pad);
std::tuple<std::string, long, long, long, long, long> gconv2d_plan(
    std::string op, long N, long C, long H, long W, long groups, long stride,
    long pad);

// gn.hip
std::vector<at::Tensor> gn_fwd(at::Tensor x, at::Tensor gamma, at::Tensor beta,
                               long G, double eps, bool fuse_relu,
                               c10::optional<at::Tensor> residual,
                               bool want_mask, long strips);
std::vector<at::Tensor> gn_bwd(at::Tensor x, at::Tensor dy, at::Tensor gamma,
                               at::Tensor mean, at::Tensor invstd,
                               at::Tensor mask, long G, bool fuse_relu,
                               bool has_residual, long strips);
std::tuple<long, long, long, long> gn_plan(long N, long C, long H, long W,
                                           long strips);

// se.hip
at::Tensor se_squeeze(at::Tensor u, long strips);
std::tuple<at::Tensor, at::Tensor> se_apply(
    at::Tensor u, at::Tensor a, c10::optional<at::Tensor> residual,
    bool fuse_relu, bool want_mask);
at::Tensor se_bwd_gate(at::Tensor dy, at::Tensor u, at::Tensor mask,
                       at::Tensor a, bool fuse_relu, long strips);
std::tuple<at::Tensor, c10::optional<at::Tensor>> se_bwd_dx(
    at::Tensor dy, at::Tensor u, at::Tensor mask, at::Tensor a, at::Tensor dz,
    bool fuse_relu, bool has_residual);
std::tuple<long, long, long, long> se_plan(long N, long C, long H, long W,
                                           long strips);

// ln.hip
std::tuple<at::Tensor, at::Tensor, at::Tensor> ln2d_fwd(
    at::Tensor x, at::Tensor gamma, at::Tensor beta, double eps, bool save,
    long blocks);
std::tuple<at::Tensor, at::Tensor, at::Tensor> ln2d_bwd(
    at::Tensor x, at::Tensor dy, at::Tensor gamma, at::Tensor mean,
    at::Tensor rstd, long blocks);
std::tuple<long, long, long, long> ln2d_plan(long M, long C, long blocks);
at::Tensor gelu_fwd(at::Tensor z);
at::Tensor gelu_bwd(at::Tensor dy, at::Tensor z);
at::Tensor lscale_fwd(at::Tensor u, at::Tensor gamma, at::Tensor resid);
std::tuple<at::Tensor, at::Tensor> lscale_bwd(at::Tensor dy, at::Tensor u,
                                              at::Tensor gamma, long blocks);

// attn.hip
std::tuple<at::Tensor, at::Tensor> attn_fwd(at::Tensor qkv, long heads,
                                            bool save);
at::Tensor attn_bwd(at::Tensor qkv, at::Tensor o, at::Tensor lse,
                    at::Tensor dO, long heads);
std::tuple<long, long, long, long, long> attn_plan(const std::string& op,
                                                   long N, long heads, long L);
at::Tensor add_pos_fwd(at::Tensor x, at::Tensor pos);

// data.hip
std::vector<at::Tensor> batch_gather_aug(at::Tensor store, at::Tensor labels,
                                         at::Tensor index, at::Tensor lut,
                                         long pad, bool hflip, long seed,
                                         long epoch);
std::vector<at::Tensor> batch_gather_cutmix(at::Tensor store, at::Tensor labels,
                                            at::Tensor index, at::Tensor lut,
                                            long pad, bool hflip, long seed,
                                            long epoch, long prob_thresh);

// comm.cpp
void register_comm(py::module_& m);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    register_comm(m);
    m.def("multi_tensor_unscale", &multi_tensor_unscale,
          "fused unscale + inf check over grad tensors; with partials also "
          "the per-chunk sums of squares of the unscaled values",
          py::arg("grads"), py::arg("found_inf"), py::arg("inv_scale"),
          py::arg("partials") = c10::nullopt);
    m.def("multi_tensor_sqsum", &multi_tensor_sqsum,
          "per-chunk sums of squares (read-only)",
          py::arg("tensors"), py::arg("partials"));
    m.def("norm_finalize", &norm_finalize,
          "partials -> out = {2-norm, clip coefficient} (+ telemetry)",
          py::arg("partials"), py::arg("n"), py::arg("max_norm"),
          py::arg("found_inf"), py::arg("out"), py::arg("stats"));
    m.def("multi_tensor_scale", &multi_tensor_scale,
          "tensors *= coef[0] in place (device coefficient)",
          py::arg("tensors"), py::arg("coef"),
          py::arg("found_inf") = c10::nullopt);
    m.attr("MT_CHUNK") = mt_chunk_elems();
    m.def("fused_sgd", &fused_sgd, "fused nesterov-momentum SGD step",
          py::arg("params"), py::arg("grads"), py::arg("bufs"), py::arg("lr"),
          py::arg("momentum"), py::arg("wd"), py::arg("nesterov"),
          py::arg("found_inf") = c10::nullopt,
          py::arg("grad_scale") = c10::nullopt);
    m.def("fused_lars", &fused_lars,
          "fused LARS step: per-tensor trust ratios (two partials per chunk, "
          "one ratio per tensor, list order) applied inside the SGD step",
          py::arg("params"), py::arg("grads"), py::arg("bufs"),
          py::arg("partials"), py::arg("ratios"), py::arg("lr"),
          py::arg("momentum"), py::arg("wd"), py::arg("nesterov"),
          py::arg("eta"), py::arg("eps"), py::arg("trust_clip"),
          py::arg("found_inf") = c10::nullopt,
          py::arg("grad_scale") = c10::nullopt);
    m.attr("ADAM_NCOEF") = adam_ncoef();
    m.def("fused_adamw", &fused_adamw,
          "fused AdamW step with a device-side step counter: steps holds one "
          "float per tensor, coefs ADAM_NCOEF per tensor (list order); both "
          "stay untouched when found_inf is set",
          py::arg("params"), py::arg("grads"), py::arg("exp_avgs"),
          py::arg("exp_avg_sqs"), py::arg("steps"), py::arg("coefs"),
          py::arg("lr"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
          py::arg("wd"), py::arg("decoupled"),
          py::arg("found_inf") = c10::nullopt,
          py::arg("grad_scale") = c10::nullopt);
    m.def("fused_lamb", &fused_lamb,
          "fused LAMB step: the AdamW counter and moments, per-tensor trust "
          "ratios |p|/|u| (two partials per chunk, one ratio per tensor)",
          py::arg("params"), py::arg("grads"), py::arg("exp_avgs"),
          py::arg("exp_avg_sqs"), py::arg("steps"), py::arg("coefs"),
          py::arg("partials"), py::arg("ratios"), py::arg("lr"),
          py::arg("beta1"), py::arg("beta2"), py::arg("eps"), py::arg("wd"),
          py::arg("trust_clip"), py::arg("max_trust"),
          py::arg("found_inf") = c10::nullopt,
          py::arg("grad_scale") = c10::nullopt);
    m.def("fused_lookahead", &fused_lookahead, "fused Lookahead interpolation",
          py::arg("fast"), py::arg("slow"), py::arg("alpha"),
          py::arg("found_inf") = c10::nullopt);
    m.def("cast_to_bf16", &cast_to_bf16);
    m.def("pad8_channels", &pad8_channels);
    m.def("nhwc_flatten", &nhwc_flatten);
    m.def("nhwc_unflatten", &nhwc_unflatten);
    m.def("pack_conv_weight", &pack_conv_weight, py::arg("w"),
          py::arg("pad8") = false, py::arg("want_wt2") = true);
    m.def("ce_fwd", &ce_fwd);
    m.def("ce_bwd", &ce_bwd);
    m.def("argmax_correct", &argmax_correct);
    m.def("ce_mix_fwd", &ce_mix_fwd,
          "CE against q = eps/C + (1-eps)(lam*onehot(a) + (1-lam)*onehot(b)): "
          "(mean loss, lse)",
          py::arg("logits"), py::arg("target_a"), py::arg("target_b"),
          py::arg("lam"), py::arg("smoothing"));
    m.def("ce_mix_bwd", &ce_mix_bwd,
          py::arg("logits"), py::arg("target_a"), py::arg("target_b"),
          py::arg("lam"), py::arg("lse"), py::arg("dloss"),
          py::arg("smoothing"));
    m.def("maxpool2x2_fwd", &maxpool2x2_fwd);
    m.def("maxpool2x2_bwd", &maxpool2x2_bwd);
    m.def("maxpool_fwd", &maxpool_fwd);
    m.def("maxpool_bwd", &maxpool_bwd);
    m.def("global_avgpool_fwd", &global_avgpool_fwd);
    m.def("global_avgpool_bwd", &global_avgpool_bwd);
    m.def("bn_fwd_train", &bn_fwd_train,
          py::arg("x"), py::arg("gamma"), py::arg("beta"),
          py::arg("running_mean"), py::arg("running_var"), py::arg("momentum"),
          py::arg("eps"), py::arg("fuse_relu") = false,
          py::arg("residual") = c10::nullopt,
          py::arg("pre_stats") = c10::nullopt);
    m.def("bn_fwd_eval", &bn_fwd_eval,
          py::arg("x"), py::arg("gamma"), py::arg("beta"),
          py::arg("running_mean"), py::arg("running_var"), py::arg("eps"),
          py::arg("fuse_relu") = false, py::arg("residual") = c10::nullopt);
    m.def("bn_bwd", &bn_bwd,
          py::arg("x"), py::arg("dy"), py::arg("gamma"), py::arg("save_mean"),
          py::arg("save_invstd"), py::arg("mask"), py::arg("fuse_relu") = false,
          py::arg("want_dresid") = false, py::arg("pre_slab") = c10::nullopt,
          py::arg("eval_stats") = false);
    m.def("bn_fwd_eval_mask", &bn_fwd_eval_mask,
          py::arg("x"), py::arg("gamma"), py::arg("beta"),
          py::arg("running_mean"), py::arg("running_var"), py::arg("eps"),
          py::arg("fuse_relu") = false, py::arg("residual") = c10::nullopt);
    m.def("bn_fwd_train_pool2", &bn_fwd_train_pool2,
          "BN(train) + ReLU + 2x2/s2 max-pool in one apply pass",
          py::arg("x"), py::arg("gamma"), py::arg("beta"),
          py::arg("running_mean"), py::arg("running_var"), py::arg("momentum"),
          py::arg("eps"), py::arg("pre_stats") = c10::nullopt);
    m.def("bn_bwd_pool2", &bn_bwd_pool2,
          py::arg("x"), py::arg("dy_pooled"), py::arg("gamma"),
          py::arg("save_mean"), py::arg("save_invstd"), py::arg("code"));
    m.def("bn_sync_local", &bn_sync_local,
          "SyncBatchNorm forward, rank-local half: [sum | sumsq | count] row",
          py::arg("x"), py::arg("pre_stats") = c10::nullopt);
    m.def("bn_sync_fwd", &bn_sync_fwd,
          "SyncBatchNorm forward, cross-rank half over gathered rows",
          py::arg("x"), py::arg("gathered"), py::arg("gamma"),
          py::arg("beta"), py::arg("running_mean"), py::arg("running_var"),
          py::arg("momentum"), py::arg("eps"), py::arg("fuse_relu") = false,
          py::arg("residual") = c10::nullopt);
    m.def("bn_sync_bwd_local", &bn_sync_bwd_local,
          "SyncBatchNorm backward, rank-local half: [dbeta | dgamma] row",
          py::arg("x"), py::arg("dy"), py::arg("save_mean"),
          py::arg("save_invstd"), py::arg("mask"),
          py::arg("fuse_relu") = false);
    m.def("bn_sync_bwd_dx", &bn_sync_bwd_dx,
          "SyncBatchNorm backward, cross-rank half over gathered rows",
          py::arg("x"), py::arg("dy"), py::arg("gamma"), py::arg("save_mean"),
          py::arg("save_invstd"), py::arg("mask"), py::arg("fuse_relu"),
          py::arg("gathered"), py::arg("count"),
          py::arg("want_dresid") = false);
    m.def("gemm_tn", &gemm_tn, py::arg("A"), py::arg("B"),
          py::arg("bias") = c10::nullopt, py::arg("out_f32") = false,
          py::arg("impl") = -1);
    m.def("transpose_bf16", &transpose_bf16);
    m.def("col_sum", &col_sum);
    m.def("linear_fwd", &linear_fwd, py::arg("x"), py::arg("w"),
          py::arg("bias") = c10::nullopt, py::arg("impl") = -1);
    m.def("linear_dgrad", &linear_dgrad, py::arg("dy"), py::arg("w"),
          py::arg("impl") = -1);
    m.def("linear_wgrad", &linear_wgrad, py::arg("dy"), py::arg("x"),
          py::arg("impl") = -1);
    m.def("linear_plan", &linear_plan,
          "'dma' or 'legacy': the GEMM a linear layer's product would run; "
          "op 0 forward, 1 dgrad, 2 wgrad, 3 a plain gemm_tn(A [M,K], B [N,K]); "
          "(M, N, K) = batch, out features, in features; impl -1 automatic, 0 legacy, 1 forces the LDS-DMA "
          "kernel where the shape fits; launches nothing",
          py::arg("op"), py::arg("M"), py::arg("N"), py::arg("K"),
          py::arg("impl") = -1);
    m.def("linear_act_fwd", &linear_act_fwd,
          "bf16 dropout(relu(x w^T + bias)) in the GEMM epilogue; thr is the "
          "drop probability in 1/65536 (0: ReLU alone), scale = "
          "65536/(65536-thr), call_seed the per-call seed's 64 bits as int64",
          py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("thr"),
          py::arg("scale"), py::arg("call_seed"), py::arg("impl") = -1);
    m.def("relu_drop_bwd", &relu_drop_bwd,
          "dz = dy*scale where the fused forward's output y > 0, else 0",
          py::arg("dy"), py::arg("y"), py::arg("scale"));
    m.def("dropout_fwd", &dropout_fwd,
          "counter-hash dropout in storage order (bf16/fp32, contiguous or "
          "channels_last)",
          py::arg("x"), py::arg("thr"), py::arg("scale"),
          py::arg("call_seed"));
    m.def("dropout_bwd", &dropout_bwd,
          "dropout backward: the same mask, regenerated, applied to dy",
          py::arg("dy"), py::arg("thr"), py::arg("scale"),
          py::arg("call_seed"));
    m.def("relu_dropout_fwd", &relu_dropout_fwd,
          "dropout_fwd over relu(x)",
          py::arg("x"), py::arg("thr"), py::arg("scale"),
          py::arg("call_seed"));
    m.def("conv2d_fwd", &conv2d_fwd, py::arg("x"), py::arg("w"),
          py::arg("bias") = c10::nullopt, py::arg("stride") = 1,
          py::arg("pad") = 0, py::arg("kwalk") = -1);
    m.def("conv2d_fwd_stats", &conv2d_fwd_stats, py::arg("x"), py::arg("w"),
          py::arg("bias") = c10::nullopt, py::arg("stride") = 1,
          py::arg("pad") = 0, py::arg("kwalk") = -1);
    m.def("conv2d_dgrad", &conv2d_dgrad,
          py::arg("dy"), py::arg("wt2"), py::arg("N"), py::arg("C"),
          py::arg("H"), py::arg("W"), py::arg("R"), py::arg("S"),
          py::arg("stride"), py::arg("pad"),
          py::arg("addend") = c10::nullopt, py::arg("group") = -1,
          py::arg("kwalk") = -1);
    m.def("conv2d_stem_fwd", &conv2d_stem_fwd,
          "C < 8 stem forward from the unpadded bf16 x and the fp32 master "
          "weight: (y, slab); slab is the [2, Ko, S] BN partial slab with "
          "want_stats, else undefined.  stem as in conv2d_stem_plan",
          py::arg("x"), py::arg("w"), py::arg("bias") = c10::nullopt,
          py::arg("stride") = 1, py::arg("pad") = 0,
          py::arg("want_stats") = false, py::arg("stem") = -1);
    m.def("conv2d_stem_plan", &conv2d_stem_plan,
          "'direct' or 'mfma': the kernel conv2d_stem_fwd would run for this "
          "shape; stem -1 automatic, 0 mfma, 1 forces direct; launches "
          "nothing",
          py::arg("N"), py::arg("C"), py::arg("H"), py::arg("W"),
          py::arg("Ko"), py::arg("R"), py::arg("S"), py::arg("stride"),
          py::arg("pad"), py::arg("stem") = -1);
    m.def("dwconv2d_fwd", &dwconv2d_fwd,
          "depthwise 3x3 forward from bf16 channels_last x and the fp32 "
          "master weight [C,1,3,3]: (y, slab); slab is the [2, C, S] BN "
          "partial slab with want_stats, else undefined",
          py::arg("x"), py::arg("w"), py::arg("bias") = c10::nullopt,
          py::arg("stride") = 1, py::arg("pad") = 0,
          py::arg("want_stats") = false, py::arg("tr") = -1);
    m.def("dwconv2d_dgrad", &dwconv2d_dgrad,
          "depthwise 3x3 backward-data: dx bf16 [N,C,H,W], every element "
          "written",
          py::arg("dy"), py::arg("w"), py::arg("H"), py::arg("W"),
          py::arg("stride") = 1, py::arg("pad") = 0, py::arg("tr") = -1);
    m.def("dwconv2d_wgrad", &dwconv2d_wgrad,
          "depthwise 3x3 backward-weight: (dw fp32 [C,1,3,3], db fp32 [C] or "
          "undefined)",
          py::arg("dy"), py::arg("x"), py::arg("stride") = 1,
          py::arg("pad") = 0, py::arg("want_db") = false,
          py::arg("tr") = -1);
    m.def("dwconv2d_plan", &dwconv2d_plan,
          "(slice width in chunks, strip rows, grid x, grid y) of the "
          "depthwise kernel for op 'fwd', 'dgrad' or 'wgrad' over an "
          "[N,C,H,W] input; launches nothing",
          py::arg("op"), py::arg("N"), py::arg("C"), py::arg("H"),
          py::arg("W"), py::arg("stride"), py::arg("pad"),
          py::arg("tr") = -1);
    m.def("dwconvk2d_fwd", &dwconvk2d_fwd,
          "depthwise 5x5 / 7x7 forward from bf16 channels_last x and the fp32 "
          "master weight [C,1,K,K]: (y, slab); slab is the [2, C, S] BN "
          "partial slab with want_stats, else undefined",
          py::arg("x"), py::arg("w"), py::arg("bias") = c10::nullopt,
          py::arg("stride") = 1, py::arg("pad") = 0,
          py::arg("want_stats") = false, py::arg("to") = -1);
    m.def("dwconvk2d_dgrad", &dwconvk2d_dgrad,
          "depthwise 5x5 / 7x7 backward-data: dx bf16 [N,C,H,W], every "
          "element written",
          py::arg("dy"), py::arg("w"), py::arg("H"), py::arg("W"),
          py::arg("stride") = 1, py::arg("pad") = 0, py::arg("to") = -1);
    m.def("dwconvk2d_wgrad", &dwconvk2d_wgrad,
          "depthwise 5x5 / 7x7 backward-weight: (dw fp32 [C,1,K,K], db fp32 "
          "[C] or undefined)",
          py::arg("dy"), py::arg("x"), py::arg("K"), py::arg("stride") = 1,
          py::arg("pad") = 0, py::arg("want_db") = false,
          py::arg("to") = -1);
    m.def("dwconvk2d_plan", &dwconvk2d_plan,
          "(slice width in chunks, rows per run / group, grid x, grid y) of "
          "the depthwise KxK kernel for op 'fwd', 'dgrad' or 'wgrad' over an "
          "[N,C,H,W] input; launches nothing",
          py::arg("op"), py::arg("N"), py::arg("C"), py::arg("H"),
          py::arg("W"), py::arg("K"), py::arg("stride"), py::arg("pad"),
          py::arg("to") = -1);
    m.def("gconv2d_pack", &gconv2d_pack,
          "grouped 3x3 weight pack: fp32 master [C,Cg,3,3] -> (forward image, "
          "dgrad image), each bf16 [C/64, 9, 64, 64]",
          py::arg("w"));
    m.def("gconv2d_fwd", &gconv2d_fwd,
          "grouped 3x3 forward from bf16 channels_last x and the forward "
          "image: (y, slab); slab is the [2, C, row tiles] BN partial slab "
          "with want_stats, else undefined",
          py::arg("x"), py::arg("wimg"), py::arg("bias") = c10::nullopt,
          py::arg("groups") = 1, py::arg("stride") = 1, py::arg("pad") = 0,
          py::arg("want_stats") = false);
    m.def("gconv2d_dgrad", &gconv2d_dgrad,
          "grouped 3x3 backward-data from dy and the dgrad image: dx bf16 "
          "[N,C,H,W], every element written",
          py::arg("dy"), py::arg("wimg_t"), py::arg("H"), py::arg("W"),
          py::arg("groups"), py::arg("stride") = 1, py::arg("pad") = 0);
    m.def("gconv2d_wgrad", &gconv2d_wgrad,
          "grouped 3x3 backward-weight: dw fp32 [C,Cg,3,3]",
          py::arg("dy"), py::arg("x"), py::arg("groups"),
          py::arg("stride") = 1, py::arg("pad") = 0);
    m.def("gconv2d_plan", &gconv2d_plan,
          "(instantiation, row tile, grid x, grid y, grid z, split) of the "
          "grouped kernel for op 'fwd', 'dgrad' or 'wgrad' over an [N,C,H,W] "
          "input; launches nothing",
          py::arg("op"), py::arg("N"), py::arg("C"), py::arg("H"),
          py::arg("W"), py::arg("groups"), py::arg("stride"), py::arg("pad"));
    m.def("gn_fwd", &gn_fwd,
          "GroupNorm forward over bf16 channels_last x with the fused "
          "relu(norm(x) + residual) epilogue: (y, mean [N,G], invstd [N,G], "
          "mask); the packed relu mask is written only with fuse_relu and "
          "want_mask; strips > 0 forces the strip count",
          py::arg("x"), py::arg("gamma"), py::arg("beta"), py::arg("G"),
          py::arg("eps"), py::arg("fuse_relu") = false,
          py::arg("residual") = c10::nullopt, py::arg("want_mask") = true,
          py::arg("strips") = -1);
    m.def("gn_bwd", &gn_bwd,
          "GroupNorm backward: (dx, dgamma, dbeta[, dresid])",
          py::arg("x"), py::arg("dy"), py::arg("gamma"), py::arg("mean"),
          py::arg("invstd"), py::arg("mask"), py::arg("G"),
          py::arg("fuse_relu") = false, py::arg("has_residual") = false,
          py::arg("strips") = -1);
    m.def("gn_plan", &gn_plan,
          "(chunks per slice, row walkers, strips, channel slices) of the "
          "GroupNorm kernels over an [N,C,H,W] input; strips > 0 forces the "
          "strip count, clamped to H*W; launches nothing",
          py::arg("N"), py::arg("C"), py::arg("H"), py::arg("W"),
          py::arg("strips") = -1);
    m.def("se_squeeze", &se_squeeze,
          "Squeeze-and-Excitation squeeze: z [N,C] bf16 = mean over (H, W) of "
          "bf16 channels_last u (fp32 sums, one division, one rounding); "
          "strips > 0 forces the strip count",
          py::arg("u"), py::arg("strips") = -1);
    m.def("se_apply", &se_apply,
          "(y, mask): y = relu?(u * sigmoid(a)[n, c] (+ residual)) for bf16 "
          "gate logits a [N,C]; the packed relu mask is written only with "
          "fuse_relu and want_mask",
          py::arg("u"), py::arg("a"), py::arg("residual") = c10::nullopt,
          py::arg("fuse_relu") = false, py::arg("want_mask") = true);
    m.def("se_bwd_gate", &se_bwd_gate,
          "da [N,C] bf16 = (sum_hw g u) s (1 - s), g the relu-masked dy",
          py::arg("dy"), py::arg("u"), py::arg("mask"), py::arg("a"),
          py::arg("fuse_relu") = false, py::arg("strips") = -1);
    m.def("se_bwd_dx", &se_bwd_dx,
          "(dx, dresid): dx = g s + dz / HW for the squeeze gradient dz "
          "[N,C]; dresid = g with a residual (dy itself without relu), else "
          "None",
          py::arg("dy"), py::arg("u"), py::arg("mask"), py::arg("a"),
          py::arg("dz"), py::arg("fuse_relu") = false,
          py::arg("has_residual") = false);
    m.def("se_plan", &se_plan,
          "(chunks per slice, row walkers, strips, channel slices) of the SE "
          "kernels over an [N,C,H,W] input; strips > 0 forces the strip "
          "count, clamped to H*W; launches nothing",
          py::arg("N"), py::arg("C"), py::arg("H"), py::arg("W"),
          py::arg("strips") = -1);
    m.def("ln2d_fwd", &ln2d_fwd,
          "LayerNorm over the C channels of every pixel of bf16 channels_last "
          "x (C % 8 == 0, C <= 2048): (y, mean [N*H*W], rstd [N*H*W]); the "
          "statistics are written only with save; blocks > 0 forces the grid",
          py::arg("x"), py::arg("gamma"), py::arg("beta"), py::arg("eps"),
          py::arg("save"), py::arg("blocks") = -1);
    m.def("ln2d_bwd", &ln2d_bwd,
          "LayerNorm backward: (dx, dgamma, dbeta)",
          py::arg("x"), py::arg("dy"), py::arg("gamma"), py::arg("mean"),
          py::arg("rstd"), py::arg("blocks") = -1);
    m.def("ln2d_plan", &ln2d_plan,
          "(lanes per row, chunks per lane, rows per group, backward grid) of "
          "the LayerNorm / layer-scale kernels over M rows of C channels; "
          "blocks > 0 forces the grid, clamped to the number of row groups; "
          "launches nothing",
          py::arg("M"), py::arg("C"), py::arg("blocks") = -1);
    m.def("gelu_fwd", &gelu_fwd,
          "a = z/2 (1 + erf(z / sqrt 2)) over a dense bf16 tensor, "
          "numel % 8 == 0", py::arg("z"));
    m.def("gelu_bwd", &gelu_bwd,
          "dz = dy (Phi(z) + z phi(z)) for the pre-activation z",
          py::arg("dy"), py::arg("z"));
    m.def("lscale_fwd", &lscale_fwd,
          "y = resid + gamma[c] * u over bf16 channels_last tensors",
          py::arg("u"), py::arg("gamma"), py::arg("resid"));
    m.def("lscale_bwd", &lscale_bwd,
          "(du, dgamma) of the layer scale; the residual's gradient is dy",
          py::arg("dy"), py::arg("u"), py::arg("gamma"),
          py::arg("blocks") = -1);
    m.def("attn_fwd", &attn_fwd,
          "softmax(q k^T / 8) v per head of 64 channels over packed bf16 "
          "channels_last qkv [N, 3*64*heads, H, W]: (o [N, 64*heads, H, W], "
          "lse [N, heads, H*W] fp32); lse is empty without save",
          py::arg("qkv"), py::arg("heads"), py::arg("save"));
    m.def("attn_bwd", &attn_bwd,
          "dqkv in qkv's packed layout from the forward's o and lse",
          py::arg("qkv"), py::arg("o"), py::arg("lse"), py::arg("do"),
          py::arg("heads"));
    m.def("attn_plan", &attn_plan,
          "(rows per block tile, streamed tile rows, grid.x, grid.y, grid.z) "
          "of op 'fwd', 'bwd_dq' or 'bwd_dkv'; launches nothing",
          py::arg("op"), py::arg("N"), py::arg("heads"), py::arg("L"));
    m.def("add_pos_fwd", &add_pos_fwd,
          "x + pos, pos [1, C, H, W] broadcast over N, bf16 channels_last",
          py::arg("x"), py::arg("pos"));
    m.def("conv2d_kloop_plan", &conv2d_kloop_plan,
          "'walk' or 'decode': the K loop conv2d_fwd[_stats] (mode 0) or "
          "conv2d_dgrad (mode 1) would run for this shape; kwalk -1 "
          "automatic, 0 decode, 1 forces the scalar tap walk; launches "
          "nothing",
          py::arg("mode"), py::arg("N"), py::arg("C"), py::arg("H"),
          py::arg("W"), py::arg("Ko"), py::arg("R"), py::arg("S"),
          py::arg("stride"), py::arg("pad"), py::arg("kwalk") = -1);
    m.def("conv2d_dgrad_plan", &conv2d_dgrad_plan,
          "(name, G, k_tiles_issued, k_tiles_raster) conv2d_dgrad would run "
          "for this shape; group -1 automatic, 0 raster, 32/64/128 forces "
          "that tap-uniform group size; launches nothing",
          py::arg("N"), py::arg("C"), py::arg("H"), py::arg("W"),
          py::arg("Ko"), py::arg("R"), py::arg("S"), py::arg("stride"),
          py::arg("pad"), py::arg("group") = -1);
    m.def("conv2d_dgrad_bn", &conv2d_dgrad_bn);
    m.def("conv2d_wgrad", &conv2d_wgrad, py::arg("dy"), py::arg("x"),
          py::arg("R"), py::arg("S"), py::arg("stride"), py::arg("pad"),
          py::arg("walk") = -1);
    m.def("conv2d_wgrad_bias", &conv2d_wgrad_bias, py::arg("dy"),
          py::arg("x"), py::arg("R"), py::arg("S"), py::arg("stride"),
          py::arg("pad"), py::arg("walk") = -1);
    m.def("conv2d_wgrad_kloop_plan", &conv2d_wgrad_kloop_plan,
          "('walk' or 'decode', dn, dp, dq): the tile loop conv2d_wgrad[_bias] "
          "would run for this shape, and the tile step S*DEPTH = dn*P*Q + "
          "dp*Q + dq of a wide_dma leaf (zeros otherwise); walk -1 automatic, "
          "0 decode, 1 forces the carried rows; launches nothing",
          py::arg("N"), py::arg("C"), py::arg("H"), py::arg("W"),
          py::arg("Ko"), py::arg("R"), py::arg("S"), py::arg("stride"),
          py::arg("pad"), py::arg("want_bias"), py::arg("walk") = -1);
    m.def("conv2d_wgrad_walk_rows", &conv2d_wgrad_walk_rows,
          "[(n, p, q, valid)] of the GEMM row split*DEPTH + chunk_row over "
          "`tiles` steps of the carried-row state; launches nothing",
          py::arg("N"), py::arg("C"), py::arg("H"), py::arg("W"),
          py::arg("Ko"), py::arg("R"), py::arg("S"), py::arg("stride"),
          py::arg("pad"), py::arg("want_bias"), py::arg("split"),
          py::arg("chunk_row"), py::arg("tiles"));
    m.def("conv2d_wgrad_plan", &conv2d_wgrad_plan,
          "(leaf name, split, fused_bias) conv2d_wgrad[_bias] would run for "
          "this shape under this process's DDPX_WGRAD_V; launches nothing",
          py::arg("N"), py::arg("C"), py::arg("H"), py::arg("W"),
          py::arg("Ko"), py::arg("R"), py::arg("S"), py::arg("stride"),
          py::arg("pad"), py::arg("want_bias"));
    m.def("batch_gather_aug", &batch_gather_aug,
          "uint8 HWC device store -> (bf16 channels_last batch, labels): "
          "gather by index + crop/flip + LUT normalise in one launch",
          py::arg("store"), py::arg("labels"), py::arg("index"),
          py::arg("lut"), py::arg("pad"), py::arg("hflip"), py::arg("seed"),
          py::arg("epoch"));
    m.def("batch_gather_cutmix", &batch_gather_cutmix,
          "batch_gather_aug with CutMix: (images, labels_a, labels_b, lam); "
          "prob_thresh is the apply probability in 1/65536",
          py::arg("store"), py::arg("labels"), py::arg("index"),
          py::arg("lut"), py::arg("pad"), py::arg("hflip"), py::arg("seed"),
          py::arg("epoch"), py::arg("prob_thresh"));
}
