// Python bindings for the pdrl_amd CDNA4 HIP kernels.
#include <torch/extension.h>

#include <vector>

std::vector<at::Tensor> seq_lstm_forward_hip(
    const at::Tensor&, const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const c10::optional<at::Tensor>&,
    const c10::optional<at::Tensor>&, const c10::optional<at::Tensor>&);
std::vector<at::Tensor> seq_lstm_backward_core_hip(
    const at::Tensor&, const c10::optional<at::Tensor>&,
    const c10::optional<at::Tensor>&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const c10::optional<at::Tensor>&);
std::vector<at::Tensor> seq_lstm_wgrad_hip(
    const at::Tensor&, const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const c10::optional<at::Tensor>&);
void seq_lstm_wgrad_out_hip(const at::Tensor&, const at::Tensor&,
                            const at::Tensor&, const at::Tensor&,
                            const at::Tensor&, const at::Tensor&, at::Tensor&,
                            at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&,
                            at::Tensor&, at::Tensor&,
                            const c10::optional<at::Tensor>&,
                            const c10::optional<at::Tensor>&,
                            const c10::optional<at::Tensor>&,
                            const c10::optional<at::Tensor>&,
                            const c10::optional<at::Tensor>&,
                            const c10::optional<at::Tensor>&, long, long,
                            double, double, double, double);
void seq_lstm_row_step_hip(
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, at::Tensor&, at::Tensor&,
    const c10::optional<at::Tensor>&, at::Tensor&, at::Tensor&, long, double,
    double, double, double, double, double, double, double, double, double,
    double);
long seq_lstm_row_step_lds_bytes(long, long, long);
long seq_lstm_row_step_split_lds_bytes(long, long, long);
bool seq_lstm_row_step_uses_split(long, long, long);
void seq_lstm_forward_multi_hip(const at::Tensor&, const at::Tensor&,
                                const at::Tensor&, const at::Tensor&,
                                const at::Tensor&, long, long, long, long);
void seq_lstm_backward_multi_hip(const at::Tensor&, const at::Tensor&,
                                 const at::Tensor&, const at::Tensor&, long,
                                 long, long, long, bool);
void seq_lstm_wgrad_multi_hip(const at::Tensor&, const at::Tensor&,
                              const at::Tensor&, long, long,
                              const c10::optional<at::Tensor>&, long, long);
void rollout_discrete_hip(
    const at::Tensor&, const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&, at::Tensor&,
    at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&,
    at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&,
    at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&, long,
    long, long, long);
void rollout_gaussian_hip(
    const at::Tensor&, const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&, at::Tensor&,
    at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&,
    at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&,
    at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&,
    at::Tensor&, long, long, long, long, long, long, long, double, double);
void rollout_eval_discrete_hip(
    const at::Tensor&, const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&, at::Tensor&,
    at::Tensor&, const c10::optional<at::Tensor>&, long, long, long);
void rollout_eval_gaussian_hip(
    const at::Tensor&, const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&, at::Tensor&,
    at::Tensor&, const c10::optional<at::Tensor>&, long, long, long);
double rollout_uniform_host(long, long, long, long);
void replay_push_sample_hip(const std::vector<at::Tensor>&,
                            const std::vector<at::Tensor>&,
                            const std::vector<at::Tensor>&, long, long, long,
                            long, long, long, long);
void seq_lstm_fwd_loss_hip(
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, at::Tensor&, at::Tensor&,
    const c10::optional<at::Tensor>&, long, double, double, double, double,
    double, double, double, double, double, double, double,
    const c10::optional<at::Tensor>&, const c10::optional<at::Tensor>&,
    const c10::optional<at::Tensor>&, const c10::optional<at::Tensor>&);
void seq_lstm_bwd_fin_hip(
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, at::Tensor&, at::Tensor&,
    at::Tensor&, at::Tensor&, long, double, double, double,
    double, const c10::optional<at::Tensor>&,
    const c10::optional<at::Tensor>&, const c10::optional<at::Tensor>&,
    const c10::optional<at::Tensor>&, const c10::optional<at::Tensor>&,
    const c10::optional<at::Tensor>&, const c10::optional<at::Tensor>&);
void onpolicy_loss_rows_hip(
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, at::Tensor&, at::Tensor&,
    const c10::optional<at::Tensor>&, long, double, double, double, double,
    double, double, double, double, double, double, double,
    const c10::optional<at::Tensor>&, const c10::optional<at::Tensor>&,
    const c10::optional<at::Tensor>&, const c10::optional<at::Tensor>&);
void onpolicy_stats_fin_hip(const at::Tensor&, at::Tensor&, long, long, long,
                            long, double, double, double, double);
void vmpo_grad_rows_hip(const at::Tensor&, const at::Tensor&,
                        const at::Tensor&, const at::Tensor&,
                        const at::Tensor&, const at::Tensor&,
                        const at::Tensor&, at::Tensor&, double, double,
                        double);
bool vmpo_mid_hip(const at::Tensor&, const at::Tensor&, const at::Tensor&,
                  const at::Tensor&, const at::Tensor&, const at::Tensor&,
                  const at::Tensor&, const at::Tensor&, at::Tensor&,
                  at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&,
                  const c10::optional<at::Tensor>&, at::Tensor&, long,
                  double, double, double, double, double, double);
at::Tensor gae_hip(const at::Tensor&, double, double, const at::Tensor&);
std::vector<at::Tensor> vtrace_hip(const at::Tensor&, const at::Tensor&,
                                   const at::Tensor&, const at::Tensor&,
                                   const at::Tensor&, double, double, double,
                                   double, long, long, double);
void sac_actor_loss_hip(const at::Tensor&, const at::Tensor&,
                        const at::Tensor&, const at::Tensor&, at::Tensor&,
                        at::Tensor&, at::Tensor&,
                        const c10::optional<at::Tensor>&,
                        const c10::optional<at::Tensor>&, double,
                        const c10::optional<at::Tensor>&, double, double);
void sac_critic_loss_hip(const at::Tensor&, const at::Tensor&,
                         const at::Tensor&, const at::Tensor&,
                         const at::Tensor&, const at::Tensor&,
                         const at::Tensor&, const at::Tensor&,
                         const at::Tensor&, at::Tensor&, at::Tensor&,
                         at::Tensor&, const c10::optional<at::Tensor>&,
                         double, double);
void sacc_sample_hip(const at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&,
                     at::Tensor&);
void sacc_actor_grad_hip(const at::Tensor&, const at::Tensor&,
                         const at::Tensor&, const at::Tensor&,
                         const at::Tensor&, const at::Tensor&,
                         const at::Tensor&, at::Tensor&, at::Tensor&,
                         at::Tensor&, const c10::optional<at::Tensor>&,
                         const c10::optional<at::Tensor>&, double,
                         const c10::optional<at::Tensor>&, double, double);
void sacc_min_mask_hip(const at::Tensor&, const at::Tensor&, at::Tensor&,
                       at::Tensor&, at::Tensor&);
void sacc_critic_loss_hip(const at::Tensor&, const at::Tensor&,
                          const at::Tensor&, const at::Tensor&,
                          const at::Tensor&, const at::Tensor&,
                          const at::Tensor&, const at::Tensor&, at::Tensor&,
                          at::Tensor&, at::Tensor&,
                          const c10::optional<at::Tensor>&, double, double);
void l2norm_sq_hip(const at::Tensor&, at::Tensor&);
void rmsprop_step_hip(at::Tensor&, const at::Tensor&, at::Tensor&,
                      const at::Tensor&, double, double, double, double);
void adam_step_hip(at::Tensor&, const at::Tensor&, at::Tensor&, at::Tensor&,
                   at::Tensor&, const at::Tensor&, double, double, double,
                   double, double, bool, const c10::optional<at::Tensor>&,
                   const c10::optional<at::Tensor>&, double,
                   const c10::optional<at::Tensor>&, double);
void sac_actor_bwd_hip(const at::Tensor&, const at::Tensor&,
                       const at::Tensor&, const at::Tensor&, at::Tensor&,
                       at::Tensor&, const c10::optional<at::Tensor>&,
                       const at::Tensor&, const at::Tensor&,
                       const at::Tensor&, const at::Tensor&,
                       const at::Tensor&, const at::Tensor&,
                       const at::Tensor&, at::Tensor&, at::Tensor&);
void sac_actor_wgrad_hip(const at::Tensor&, const at::Tensor&,
                         const at::Tensor&, const at::Tensor&,
                         const at::Tensor&, const at::Tensor&, at::Tensor&,
                         at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&,
                         at::Tensor&, at::Tensor&,
                         const c10::optional<at::Tensor>&, const at::Tensor&,
                         const at::Tensor&, at::Tensor&, at::Tensor&,
                         const c10::optional<at::Tensor>&,
                         const c10::optional<at::Tensor>&, double, double,
                         double);
void sac_fwd2_critic_loss_hip(
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, at::Tensor&, at::Tensor&,
    at::Tensor&, const c10::optional<at::Tensor>&, double, double);
void sacc_fwd_sample_hip(
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&,
    at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&,
    const c10::optional<at::Tensor>&, const c10::optional<at::Tensor>&,
    const c10::optional<at::Tensor>&);
void sacc_minmask_bwd_hip(
    const at::Tensor&, const at::Tensor&, at::Tensor&, at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&, at::Tensor&,
    at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&, long);
void sacc_actor_bwd_hip(
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, at::Tensor&, at::Tensor&,
    const c10::optional<at::Tensor>&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, at::Tensor&, at::Tensor&);
void sacc_critic_bwd_hip(
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, at::Tensor&, at::Tensor&,
    at::Tensor&, const c10::optional<at::Tensor>&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&, at::Tensor&,
    at::Tensor&, at::Tensor&, at::Tensor&, double, double);
void adam_prep_hip(at::Tensor&, double, double);
void adam_multi_hip(const at::Tensor&, const at::Tensor&, const at::Tensor&,
                    long, long, double, double, double);
void soft_update_hip(const std::vector<at::Tensor>&,
                     const std::vector<at::Tensor>&, double);
void soft_update_cached_hip(const at::Tensor&, const at::Tensor&,
                            const at::Tensor&, long, long, double);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("seq_lstm_forward", &seq_lstm_forward_hip,
        "fused body+LSTM+heads forward (gfx950); dual-body via x2/body2",
        py::arg("x"), py::arg("h0"), py::arg("c0"), py::arg("body_w"),
        py::arg("body_b"), py::arg("w_ih"), py::arg("w_hh"), py::arg("b_g"),
        py::arg("heads_w"), py::arg("heads_b"), py::arg("x2") = c10::nullopt,
        py::arg("body2_w") = c10::nullopt, py::arg("body2_b") = c10::nullopt);
  m.def("seq_lstm_backward_core", &seq_lstm_backward_core_hip,
        "fused BPTT backward core (gfx950); dual-body adds dx2",
        py::arg("gouts"), py::arg("ghS"), py::arg("gcS"), py::arg("stash"),
        py::arg("x"), py::arg("c0"), py::arg("body_w"), py::arg("w_ih"),
        py::arg("w_hh"), py::arg("heads_w"),
        py::arg("body2_w") = c10::nullopt);
  m.def("seq_lstm_wgrad", &seq_lstm_wgrad_hip,
        "MFMA weight-gradient GEMMs + wave-per-element small grads",
        py::arg("x"), py::arg("h0"), py::arg("stash"), py::arg("dgates"),
        py::arg("dxb"), py::arg("gouts"), py::arg("x2") = c10::nullopt);
  m.def("seq_lstm_wgrad_out", &seq_lstm_wgrad_out_hip,
        "wgrad writing into caller buffers (flat grad views)",
        py::arg("x"), py::arg("h0"), py::arg("stash"), py::arg("dgates"),
        py::arg("dxb"), py::arg("gouts"), py::arg("dw_ih"), py::arg("dw_hh"),
        py::arg("dbody_w"), py::arg("dbody_b"), py::arg("db_g"),
        py::arg("dheads_w"), py::arg("dheads_b"), py::arg("norm_sq"),
        py::arg("x2") = c10::nullopt, py::arg("dbody2_w") = c10::nullopt,
        py::arg("dbody2_b") = c10::nullopt,
        // on-policy row step: reduce the per-row loss partials into the
        // stats vector in one extra block
        py::arg("stats_part") = c10::nullopt, py::arg("stats") = c10::nullopt,
        py::arg("algo") = 0, py::arg("B") = 0, py::arg("cp") = 0.0,
        py::arg("cv") = 0.0, py::arg("ce") = 0.0, py::arg("creg") = 0.0);
  m.def("seq_lstm_forward_multi", &seq_lstm_forward_multi_hip,
        "multi-network fused forward (device pointer tables; dual-body "
        "rows carry body2/x2 pointers)",
        py::arg("x"), py::arg("h0"), py::arg("c0"), py::arg("core_tab"),
        py::arg("out_tab"), py::arg("C"), py::arg("D"), py::arg("F2") = 0,
        py::arg("half") = 0);
  m.def("seq_lstm_backward_multi", &seq_lstm_backward_multi_hip,
        "multi-network fused backward (leaf inputs; dgates/dxb [+ dx2])",
        py::arg("x"), py::arg("c0"), py::arg("in_tab"), py::arg("out_tab"),
        py::arg("C"), py::arg("D"), py::arg("F2") = 0, py::arg("half") = 0,
        py::arg("accum_dx2") = false);
  m.def("seq_lstm_wgrad_multi", &seq_lstm_wgrad_multi_hip,
        "multi-network MFMA weight grads (device pointer table; dual-body "
        "encoder grad segments)",
        py::arg("x"), py::arg("h0"), py::arg("tab"), py::arg("C"),
        py::arg("D"), py::arg("x2") = c10::nullopt, py::arg("F2") = 0,
        py::arg("half") = 0);
  m.def("rollout_discrete", &rollout_discrete_hip,
        "device actor: N envs x S steps of policy-act + env-step in one "
        "launch, writing the learner's (N,S,.) batch fields in place",
        py::arg("body_w"), py::arg("body_b"), py::arg("w_ih"), py::arg("w_hh"),
        py::arg("b_g"), py::arg("heads_w"), py::arg("heads_b"),
        py::arg("env_state"), py::arg("h"), py::arg("c"), py::arg("is_fir"),
        py::arg("ep_steps"), py::arg("ep_run"), py::arg("tick"),
        py::arg("obs"), py::arg("act"), py::arg("rew"), py::arg("logits"),
        py::arg("log_prob"), py::arg("is_fir_out"), py::arg("hx"),
        py::arg("cx"), py::arg("ep_ret"), py::arg("env_id"), py::arg("seed"),
        py::arg("time_horizon"), py::arg("max_episode_steps"));
  m.def("rollout_gaussian", &rollout_gaussian_hip,
        "device actor for continuous control: rollout_discrete's contract "
        "with a Gaussian policy (mode 0 = PPO-C, 1 = SAC-C + OU exploration)",
        py::arg("body_w"), py::arg("body_b"), py::arg("w_ih"), py::arg("w_hh"),
        py::arg("b_g"), py::arg("heads_w"), py::arg("heads_b"),
        py::arg("env_state"), py::arg("h"), py::arg("c"), py::arg("is_fir"),
        py::arg("ep_steps"), py::arg("ep_run"), py::arg("tick"),
        py::arg("ou_state"), py::arg("obs"), py::arg("act"), py::arg("rew"),
        py::arg("logits"), py::arg("log_prob"), py::arg("is_fir_out"),
        py::arg("hx"), py::arg("cx"), py::arg("ep_ret"), py::arg("env_id"),
        py::arg("mode"), py::arg("seed"), py::arg("time_horizon"),
        py::arg("max_episode_steps"), py::arg("ou_envs"),
        py::arg("warmup_steps"), py::arg("ou_theta"), py::arg("ou_sigma"));
  m.def("rollout_eval_discrete", &rollout_eval_discrete_hip,
        "greedy evaluation: E whole episodes per env under the arg-max "
        "action in one launch; writes ep_ret / ep_len (N, E) only",
        py::arg("body_w"), py::arg("body_b"), py::arg("w_ih"), py::arg("w_hh"),
        py::arg("b_g"), py::arg("heads_w"), py::arg("heads_b"),
        py::arg("ep_ret"), py::arg("ep_len"), py::arg("start_state"),
        py::arg("env_id"), py::arg("seed"), py::arg("max_episode_steps"));
  m.def("rollout_eval_gaussian", &rollout_eval_gaussian_hip,
        "greedy evaluation for continuous control: rollout_eval_discrete's "
        "contract with the action tanh(mu)",
        py::arg("body_w"), py::arg("body_b"), py::arg("w_ih"), py::arg("w_hh"),
        py::arg("b_g"), py::arg("heads_w"), py::arg("heads_b"),
        py::arg("ep_ret"), py::arg("ep_len"), py::arg("start_state"),
        py::arg("env_id"), py::arg("seed"), py::arg("max_episode_steps"));
  m.def("rollout_uniform", &rollout_uniform_host,
        "host evaluation of the rollout's counter-hash uniform",
        py::arg("seed"), py::arg("env"), py::arg("tick"), py::arg("k"));
  m.def("replay_push_sample", &replay_push_sample_hip,
        "device replay: append n_push source rows to the per-field rings and "
        "gather n_sample hash-drawn trajectories into out, in one launch "
        "(observably push, then sample)",
        py::arg("src"), py::arg("ring"), py::arg("out"), py::arg("n_push"),
        py::arg("n_sample"), py::arg("head"), py::arg("capacity"),
        py::arg("filled"), py::arg("draw"), py::arg("seed"));
  m.def("seq_lstm_fwd_loss", &seq_lstm_fwd_loss_hip,
        "forward + row-local loss (IMPALA/PPO/PPO-C, V-MPO pre) in ONE "
        "launch",
        py::arg("x"), py::arg("h0"), py::arg("c0"), py::arg("body_w"),
        py::arg("body_b"), py::arg("w_ih"), py::arg("w_hh"), py::arg("b_g"),
        py::arg("heads_w"), py::arg("heads_b"), py::arg("outs"),
        py::arg("hS"), py::arg("cS"), py::arg("stash"), py::arg("act"),
        py::arg("behav"), py::arg("rew"), py::arg("fir"), py::arg("gouts"),
        py::arg("stats_part"), py::arg("norm_sq"), py::arg("algo"),
        py::arg("gamma"), py::arg("lmbda"), py::arg("rho_bar"),
        py::arg("rho_min"), py::arg("c_bar"), py::arg("rew_scale"),
        py::arg("cp"), py::arg("cv"), py::arg("ce"), py::arg("eps_clip"),
        py::arg("creg"), py::arg("vm_lse") = c10::nullopt,
        py::arg("vm_logp") = c10::nullopt, py::arg("vm_adv") = c10::nullopt,
        py::arg("vm_td") = c10::nullopt);
  m.def("seq_lstm_row_step", &seq_lstm_row_step_hip,
        "forward + row-local loss + BPTT (IMPALA/PPO/PPO-C) in ONE launch",
        py::arg("x"), py::arg("h0"), py::arg("c0"), py::arg("body_w"),
        py::arg("body_b"), py::arg("w_ih"), py::arg("w_hh"), py::arg("b_g"),
        py::arg("heads_w"), py::arg("heads_b"), py::arg("outs"),
        py::arg("hS"), py::arg("cS"), py::arg("stash"), py::arg("act"),
        py::arg("behav"), py::arg("rew"), py::arg("fir"), py::arg("gouts"),
        py::arg("stats_part"), py::arg("norm_sq"), py::arg("dgates"),
        py::arg("dxb"), py::arg("algo"), py::arg("gamma"), py::arg("lmbda"),
        py::arg("rho_bar"), py::arg("rho_min"), py::arg("c_bar"),
        py::arg("rew_scale"), py::arg("cp"), py::arg("cv"), py::arg("ce"),
        py::arg("eps_clip"), py::arg("creg"));
  m.def("seq_lstm_row_step_lds_bytes", &seq_lstm_row_step_lds_bytes,
        "dynamic LDS one seq_lstm_row_step block needs (launch limit 64 KiB)",
        py::arg("S"), py::arg("D"), py::arg("algo"));
  m.def("seq_lstm_row_step_split_lds_bytes",
        &seq_lstm_row_step_split_lds_bytes,
        "dynamic LDS of the row step with the input projections computed "
        "ahead of the forward's time loop and the head weights in LDS",
        py::arg("S"), py::arg("D"), py::arg("algo"));
  m.def("seq_lstm_row_step_uses_split", &seq_lstm_row_step_uses_split,
        "whether seq_lstm_row_step launches that instantiation (its LDS "
        "fits a launch)",
        py::arg("S"), py::arg("D"), py::arg("algo"));
  m.def("seq_lstm_bwd_fin", &seq_lstm_bwd_fin_hip,
        "BPTT backward + stat finalization (or V-MPO grad emission)",
        py::arg("gouts"), py::arg("stash"), py::arg("x"), py::arg("c0"),
        py::arg("body_w"), py::arg("w_ih"), py::arg("w_hh"),
        py::arg("heads_w"), py::arg("dgates"), py::arg("dxb"),
        py::arg("stats"), py::arg("stats_part"), py::arg("algo"),
        py::arg("cp"), py::arg("cv"), py::arg("ce"), py::arg("creg"),
        py::arg("act") = c10::nullopt, py::arg("behav") = c10::nullopt,
        py::arg("vm_lse") = c10::nullopt, py::arg("vm_psi") = c10::nullopt,
        py::arg("vm_td") = c10::nullopt,
        py::arg("vm_scalars") = c10::nullopt,
        py::arg("vm_outs") = c10::nullopt);
  m.def("onpolicy_loss_rows", &onpolicy_loss_rows_hip,
        "row-local loss (IMPALA/PPO/PPO-C, V-MPO pre) over the outputs of "
        "seq_lstm_forward, one block per batch row",
        py::arg("outs"), py::arg("act"), py::arg("behav"), py::arg("rew"),
        py::arg("fir"), py::arg("gouts"), py::arg("stats_part"),
        py::arg("norm_sq"), py::arg("algo"), py::arg("gamma"),
        py::arg("lmbda"), py::arg("rho_bar"), py::arg("rho_min"),
        py::arg("c_bar"), py::arg("rew_scale"), py::arg("cp"), py::arg("cv"),
        py::arg("ce"), py::arg("eps_clip"), py::arg("creg"),
        py::arg("vm_lse") = c10::nullopt, py::arg("vm_logp") = c10::nullopt,
        py::arg("vm_adv") = c10::nullopt, py::arg("vm_td") = c10::nullopt);
  m.def("onpolicy_stats_fin", &onpolicy_stats_fin_hip,
        "one-block reduce of the per-row loss partials into the stats vector",
        py::arg("stats_part"), py::arg("stats"), py::arg("algo"),
        py::arg("B"), py::arg("S"), py::arg("D"), py::arg("cp"),
        py::arg("cv"), py::arg("ce"), py::arg("creg"));
  m.def("vmpo_grad_rows", &vmpo_grad_rows_hip,
        "V-MPO packed head grads from vmpo_mid's psi weights, one block per "
        "batch row",
        py::arg("outs"), py::arg("act"), py::arg("behav"), py::arg("vm_lse"),
        py::arg("vm_psi"), py::arg("vm_td"), py::arg("vm_scalars"),
        py::arg("gouts"), py::arg("cp"), py::arg("cv"), py::arg("creg"));
  m.def("vmpo_mid", &vmpo_mid_hip,
        "V-MPO cross-row middle kernel: selection + psi + duals + stats");
  m.def("gae", &gae_hip, "GAE reverse scan");
  m.def("vtrace", &vtrace_hip, "fused V-trace scan",
        pybind11::arg("behav_lp"), pybind11::arg("target_lp"),
        pybind11::arg("is_fir"), pybind11::arg("rew"), pybind11::arg("val"),
        pybind11::arg("gamma"), pybind11::arg("rho_bar"),
        pybind11::arg("rho_min"), pybind11::arg("c_bar"),
        pybind11::arg("vD") = 1, pybind11::arg("val_off") = 0,
        pybind11::arg("rew_scale") = 1.0);
  m.def("sac_actor_loss", &sac_actor_loss_hip,
        "SAC discrete actor+alpha loss with analytic grads",
        py::arg("moA"), py::arg("q1"), py::arg("q2"), py::arg("log_alpha"),
        py::arg("gouts"), py::arg("g_alpha"), py::arg("stats"),
        py::arg("actor_norm"), py::arg("alpha_norm"),
        py::arg("target_entropy"), py::arg("clock") = c10::nullopt,
        py::arg("beta1") = 0.9, py::arg("beta2") = 0.999);
  m.def("sac_critic_loss", &sac_critic_loss_hip,
        "SAC discrete soft-Q target + twin critic loss grads");
  m.def("sac_actor_bwd", &sac_actor_bwd_hip,
        "SAC discrete actor loss (row-local) fused into the actor BPTT "
        "launch; per-row {ubar, entropy} partials to stats_part");
  m.def("sac_actor_wgrad", &sac_actor_wgrad_hip,
        "actor MFMA wgrad + actor-loss cross-row reduce (g_alpha, stats, "
        "alpha_norm, shared Adam clock prep) in one extra block",
        py::arg("x"), py::arg("h0"), py::arg("stash"), py::arg("dgates"),
        py::arg("dxb"), py::arg("gouts"), py::arg("dw_ih"), py::arg("dw_hh"),
        py::arg("dbody_w"), py::arg("dbody_b"), py::arg("db_g"),
        py::arg("dheads_w"), py::arg("dheads_b"), py::arg("norm_sq"),
        py::arg("stats_part"), py::arg("log_alpha"), py::arg("g_alpha"),
        py::arg("stats4"), py::arg("alpha_norm") = c10::nullopt,
        py::arg("clock") = c10::nullopt, py::arg("target_entropy") = 0.0,
        py::arg("beta1") = 0.9, py::arg("beta2") = 0.999);
  m.def("sac_fwd2_critic_loss", &sac_fwd2_critic_loss_hip,
        "post-update actor forward + SAC critic loss in one launch "
        "(fwd+loss pattern; vl partials reduced by the critic Adam)");
  m.def("sacc_sample", &sacc_sample_hip,
        "reparameterized tanh-Gaussian sample + log-prob (graph-safe RNG)");
  m.def("sacc_actor_grad", &sacc_actor_grad_hip,
        "SAC-continuous actor+alpha loss with analytic dmu/dlog_std",
        py::arg("moA"), py::arg("eps"), py::arg("act"), py::arg("g"),
        py::arg("q1"), py::arg("q2"), py::arg("log_alpha"), py::arg("dmoA"),
        py::arg("g_alpha"), py::arg("stats"), py::arg("actor_norm"),
        py::arg("alpha_norm"), py::arg("target_entropy"),
        py::arg("clock") = c10::nullopt, py::arg("beta1") = 0.9,
        py::arg("beta2") = 0.999);
  m.def("sacc_critic_loss", &sacc_critic_loss_hip,
        "SAC-continuous soft-Q target + twin critic loss grads");
  m.def("sacc_fwd_sample", &sacc_fwd_sample_hip,
        "actor forward + reparameterized tanh-Gaussian sample in one "
        "launch (optional dQ/da zeroing and behaviour-action staging)",
        py::arg("x"), py::arg("h0"), py::arg("c0"), py::arg("body_w"),
        py::arg("body_b"), py::arg("w_ih"), py::arg("w_hh"), py::arg("b_g"),
        py::arg("heads_w"), py::arg("heads_b"), py::arg("moA"),
        py::arg("hS"), py::arg("cS"), py::arg("stash"), py::arg("rng"),
        py::arg("eps"), py::arg("act"), py::arg("logpi"),
        py::arg("dact_zero") = c10::nullopt,
        py::arg("act_src") = c10::nullopt, py::arg("actb") = c10::nullopt);
  m.def("sacc_minmask_bwd", &sacc_minmask_bwd_hip,
        "min-critic selection + twin-critic input-grad backward in one "
        "launch (dminQ/da accumulated into the shared buffer)");
  m.def("sacc_actor_bwd", &sacc_actor_bwd_hip,
        "SAC-continuous analytic actor grad + actor BPTT in one launch; "
        "per-row partials reduced by sac_actor_wgrad");
  m.def("sacc_critic_bwd", &sacc_critic_bwd_hip,
        "SAC-continuous soft-Q critic loss + twin BPTT in one launch; "
        "huber partials reduced by the critic Adam");
  m.def("sacc_min_mask", &sacc_min_mask_hip,
        "min-critic selection masks for dE[-minQ]/dq + zero the dQ/da "
        "accumulator");
  m.def("l2norm_sq", &l2norm_sq_hip, "squared L2 norm into a device scalar");
  m.def("rmsprop_step", &rmsprop_step_hip, "fused clip+RMSprop on flat buffers");
  m.def("adam_step", &adam_step_hip,
        "fused clip+Adam on flat buffers (optional per-row stats reduce in "
        "block 0 and inline Polyak target tracking)",
        py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"),
        py::arg("state3"), py::arg("norm_sq"), py::arg("lr"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("max_norm"),
        py::arg("do_prep") = true, py::arg("stats_part") = c10::nullopt,
        py::arg("stats_out") = c10::nullopt, py::arg("part_scale") = 1.0,
        py::arg("polyak") = c10::nullopt, py::arg("tau") = 0.0);
  m.def("adam_prep", &adam_prep_hip,
        "advance the shared device Adam step clock");
  m.def("adam_multi", &adam_multi_hip,
        "multi-group fused clip+Adam (shared step clock, pointer table)");
  m.def("soft_update", &soft_update_hip, "multi-tensor Polyak update");
  m.def("soft_update_cached", &soft_update_cached_hip,
        "Polyak update with prebuilt device pointer tables (graph-safe)");
}
