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
                   bool out_f32);
at::Tensor transpose_bf16(at::Tensor x);
at::Tensor col_sum(at::Tensor x);
at::Tensor linear_fwd(at::Tensor x, at::Tensor w, c10::optional<at::Tensor> bias);
at::Tensor linear_dgrad(at::Tensor dy, at::Tensor w);
at::Tensor linear_wgrad(at::Tensor dy, at::Tensor x);
at::Tensor linear_act_fwd(at::Tensor x, at::Tensor w,
                          c10::optional<at::Tensor> bias, long thr,
                          double scale, long call_seed);
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
                        long stride, long pad);
std::vector<at::Tensor> conv2d_wgrad_bias(at::Tensor dy, at::Tensor x,
                                          long R, long S, long stride,
                                          long pad);
std::tuple<std::string, long, bool> conv2d_wgrad_plan(
    long N, long C, long H, long W, long Ko, long R, long S, long stride,
    long pad, bool want_bias);

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
          py::arg("bias") = c10::nullopt, py::arg("out_f32") = false);
    m.def("transpose_bf16", &transpose_bf16);
    m.def("col_sum", &col_sum);
    m.def("linear_fwd", &linear_fwd, py::arg("x"), py::arg("w"),
          py::arg("bias") = c10::nullopt);
    m.def("linear_dgrad", &linear_dgrad);
    m.def("linear_wgrad", &linear_wgrad);
    m.def("linear_act_fwd", &linear_act_fwd,
          "bf16 dropout(relu(x w^T + bias)) in the GEMM epilogue; thr is the "
          "drop probability in 1/65536 (0: ReLU alone), scale = "
          "65536/(65536-thr), call_seed the per-call seed's 64 bits as int64",
          py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("thr"),
          py::arg("scale"), py::arg("call_seed"));
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
    m.def("conv2d_wgrad", &conv2d_wgrad);
    m.def("conv2d_wgrad_bias", &conv2d_wgrad_bias);
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
