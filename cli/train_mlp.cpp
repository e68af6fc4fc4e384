// cli/train_mlp.cpp -- sshmt/main_train_sshmt_mlp.cxx and main_train_sshmt_logsig.cxx: one source for four tools, on the GPU.
// GLIA_TRAIN_LOGSIG fixes the hidden layers at 0 / 0 (train_logsig, train_sshmt_logsig: the logsig model); GLIA_TRAIN_SSHMT adds the
// merge-path (unsupervised) term on the merge paths of unlabelled volumes (train_sshmt_mlp, train_sshmt_logsig).
//   train_mlp --sl labels... --sf feats... [--im model] [--nn1 10 --nn2 10] --wr w --ws w --ss sigma [--uss 1] [--topt 1|2|3] --lr step
//             [--lrd decay] [--lrdi n] [--lrds n] --tw iterations --ts rounds [--si n] --omp pattern [--v 1] [--seed s] [--fmm minmax]
//   train_sshmt_mlp [--sl labels... --sf feats...] [--uo orders... --uf feats...] --wu w --su sigma [--usu 1] and train_mlp's other flags
// Flags and defaults are the reference's (main_train_sshmt_mlp.cxx:171-236); --seed keys this library's initial weights and --fmm
// rescales the rows inside, as pred_mlp --fmm does (the reference expects normalize_sample to have run).  --omp is a printf pattern
// taking the round index; a model is written every --si rounds and after the last.  --v 1 (the default) prints the reference's "gd:"
// and "learn-" lines from the trace.  train_mlp and train_logsig are not named train_sshmt_*: they train without the semi-supervised
// term -- --uo, --uf, a non-zero --wu, --bsu and --usu 1 end with a message naming the flag and exit status 1.
// train_sshmt_*: --uo / --uf come in equal numbers: file k of --uf holds one row per merge of file k of --uo (bc_feat's output for that
// order).  --sl / --sf may be left out when --ws is 0.
// Mini-batches are an opt-in: with --bseed S the reference's --bss B (batches of labelled rows), --bb 1 (balanced by
// class), --bsu B (train_sshmt_*: batches of merge paths), --te E (epochs per iteration, 1) and --tb N (batches per iteration when
// --te is 0, 1) are honoured, with THIS library's sampler: its permutations are a function of S, not the reference's rand() sequence.
// Without --bseed, --bsu > 0, --bss > 0, --bb 1 and (train_sshmt_*) --te / --tb other than 1 end with a message naming the flag and
// exit status 1.
#include <climits>

#include "common.hpp"

using namespace cli;

#ifdef GLIA_TRAIN_SSHMT
#define TOOL_PREFIX "train_sshmt_"
#else
#define TOOL_PREFIX "train_"
#endif
#ifdef GLIA_TRAIN_LOGSIG
static const char* const kTool = TOOL_PREFIX "logsig";
#else
static const char* const kTool = TOOL_PREFIX "mlp";
#endif

int main(int argc, char* argv[]) {
#ifdef GLIA_TRAIN_SSHMT
  const std::string usage = std::string("Usage: ") + kTool + " [--sl <labels>... --sf <feats>...] [--uo <orders>... --uf <feats>...] [--im <model>] "
#else
  const std::string usage = std::string("Usage: ") + kTool + " --sl <labels>... --sf <feats>... [--im <model>] "
#endif
#ifndef GLIA_TRAIN_LOGSIG
                            "[--nn1 <N>] [--nn2 <N>] "
#endif
#ifdef GLIA_TRAIN_SSHMT
                            "[--wr <w>] [--wu <w>] [--ws <w>] [--su <sigma>] [--ss <sigma>] [--usu <0|1>] [--uss <0|1>] [--topt <1|2|3>] [--lr <step>] "
                            "[--lrd <decay>] [--lrdi <n>] [--lrds <n>] [--tw <iterations>] [--ts <rounds>] [--si <n>] --omp <pattern> [--v <0|1>] "
                            "[--seed <s>] [--fmm <minmax>] [--bseed <S> [--bss <B>] [--bb <0|1>] [--bsu <B>] [--te <epochs>] [--tb <batches>]]\n"
                            "  (flags as sshmt/main_train_sshmt_mlp.cxx:171-236; --bsu --bss --bb, --te / --tb other than 1 need --bseed: this tool's own sampler)\n";
#else
                            "[--wr <w>] [--ws <w>] [--ss <sigma>] [--uss <0|1>] [--topt <1|2|3>] [--lr <step>] [--lrd <decay>] [--lrdi <n>] "
                            "[--lrds <n>] [--tw <iterations>] [--ts <rounds>] [--si <n>] --omp <pattern> [--v <0|1>] [--seed <s>] [--fmm <minmax>]\n"
                            "  [--bseed <S> [--bss <B>] [--bb <0|1>] [--te <epochs>] [--tb <batches>]]\n"
                            "  (flags as sshmt/main_train_sshmt_mlp.cxx:171-236; not supported: --uo --uf --wu --bsu --usu; --bss --bb need --bseed: this tool's own sampler)\n";
#endif
  Args a = parse(argc, argv, {}, {"sl", "sf", "im", "nn1", "nn2", "wr", "ws", "ss", "uss", "topt", "lr", "lrd", "lrdi", "lrds", "tw", "ts", "si", "omp", "v",
                                  "seed", "fmm", "uo", "uf", "wu", "su", "usu", "bsu", "bss", "bb", "te", "tb", "bseed"}, usage);
  const bool batches = a.has("bseed");      // the opt-in to this library's sampler
  auto refuse = [&](const char* flag, const char* what) { perr(std::string("Error: ") + kTool + ": --" + flag + " is not supported (" + what + ")"); };
#ifdef GLIA_TRAIN_SSHMT
  if (!batches && a.has("bsu") && atoi(a.str("bsu", "-1").c_str()) > 0) refuse("bsu", "batch samplers");
  if (!batches && a.has("bss") && atoi(a.str("bss", "-1").c_str()) > 0) refuse("bss", "batch samplers");
  if (!batches && flagOf(a, "bb")) refuse("bb", "batch samplers");
  if (!batches && a.has("te") && atoi(a.str("te", "1").c_str()) != 1) refuse("te", "batch samplers");
  if (!batches && a.has("tb") && atoi(a.str("tb", "1").c_str()) != 1) refuse("tb", "batch samplers");
  for (const char* req : {"omp"})
#else
  if (a.has("uo")) refuse("uo", "the unsupervised term");
  if (a.has("uf")) refuse("uf", "the unsupervised term");
  if (a.has("wu") && std::fabs(atof(a.str("wu", "0").c_str())) >= 2.22e-16) refuse("wu", "the unsupervised term");
  if (a.has("bsu")) refuse("bsu", "batch samplers");
  if (!batches && a.has("bss") && atoi(a.str("bss", "-1").c_str()) > 0) refuse("bss", "batch samplers");
  if (!batches && flagOf(a, "bb")) refuse("bb", "batch samplers");
  if (flagOf(a, "usu")) refuse("usu", "the unsupervised term");
  for (const char* req : {"sl", "sf", "omp"})
#endif
    if (!a.has(req) || a.all(req).empty()) { std::cerr << "Error: the option '--" << req << "' is required but missing\n" << usage; return EXIT_FAILURE; }
  glia_hmt_sshmt_train_opts so;
  glia_hmt_sshmt_train_opts_default(&so);
  glia_hmt_mlp_train_opts& o = so.base;
#ifdef GLIA_TRAIN_LOGSIG
  o.n1 = o.n2 = 0;
#else
  o.n1 = atoi(a.str("nn1", "10").c_str()); o.n2 = atoi(a.str("nn2", "10").c_str());
#endif
  o.wr = atof(a.str("wr", "0").c_str()); o.ws = atof(a.str("ws", "0").c_str()); o.sigma_s = atof(a.str("ss", "0").c_str());
  o.update_sigma_s = flagOf(a, "uss");
#ifdef GLIA_TRAIN_SSHMT
  o.wu = atof(a.str("wu", "0").c_str()); so.sigma_u = atof(a.str("su", "0").c_str());
  o.update_sigma_u = flagOf(a, "usu");
#endif
  o.optimizer = atoi(a.str("topt", "1").c_str());
  o.step = atof(a.str("lr", "0").c_str()); o.step_decay = atof(a.str("lrd", "1").c_str());
  o.fixed_step_decay_iterations = atoi(a.str("lrdi", "-1").c_str()); o.sigma_update_step_period = atoi(a.str("lrds", "-1").c_str());
  o.max_iterations = atoi(a.str("tw", "0").c_str()); o.n_sigma_updates = atoi(a.str("ts", "0").c_str());
  o.seed = strtoull(a.str("seed", "0").c_str(), nullptr, 0);
  glia_hmt_batch_opts bo;
  glia_hmt_batch_opts_default(&bo);
  if (batches) {
    bo.seed = strtoull(a.str("bseed").c_str(), nullptr, 0);
    bo.epochs_per_iteration = atoi(a.str("te", "1").c_str()); bo.batches_per_iteration = atoi(a.str("tb", "1").c_str());
    o.sup_batch_size = atoi(a.str("bss", "-1").c_str()); o.balance_sup_batch = flagOf(a, "bb");
#ifdef GLIA_TRAIN_SSHMT
    o.uns_batch_size = atoi(a.str("bsu", "-1").c_str());
#endif
  }
  const int saveInterval = a.has("si") ? atoi(a.str("si").c_str()) : INT_MAX;
  const bool verbose = a.has("v") ? flagOf(a, "v") : true;
  const std::string pattern = a.str("omp");

  const auto featFiles = a.has("sf") ? a.all("sf") : std::vector<std::string>(), labelFiles = a.has("sl") ? a.all("sl") : std::vector<std::string>();
#ifdef GLIA_TRAIN_SSHMT
  const auto unsFeatFiles = a.has("uf") ? a.all("uf") : std::vector<std::string>(), orderFiles = a.has("uo") ? a.all("uo") : std::vector<std::string>();
  if (unsFeatFiles.size() != orderFiles.size())
    perr(std::string("Error: ") + kTool + ": --uo and --uf must come in equal numbers (" + std::to_string(orderFiles.size()) + " and " + std::to_string(unsFeatFiles.size()) + ")");
  if (std::fabs(o.ws) >= 2.22e-16 && (featFiles.empty() || labelFiles.empty())) perr(std::string("Error: ") + kTool + ": --sl and --sf are required unless --ws is 0");
#endif
  // the rows of all feature files in file order, the labels of all label files (sshmt_util.hxx:11-27)
  std::vector<double> rows;
  std::vector<int32_t> labels;
  int dim = 0;
  for (auto& f : featFiles) {
    int64_t r = 0;
    int d = 0;
    const std::vector<double> x = readRows(f, &r, &d);
    if (r > 0 && dim > 0 && d != dim) perr("Error: invalid data file dimension in " + f);
    if (r > 0) dim = d;
    rows.insert(rows.end(), x.begin(), x.end());
  }
  for (auto& f : labelFiles) {
    std::ifstream is(f);
    if (!is) perr("Error: cannot open file " + f);
    long long v;
    while (is >> v) labels.push_back((int32_t)v);
  }
#ifdef GLIA_TRAIN_SSHMT
  // one block per (--uo, --uf) pair (sshmt_util.hxx:30-52)
  std::vector<std::vector<double>> urows(orderFiles.size());
  std::vector<std::vector<uint32_t>> orders(orderFiles.size());
  std::vector<glia_hmt_sshmt_block> blocks(orderFiles.size());
  for (size_t b = 0; b < orderFiles.size(); ++b) {
    orders[b] = readOrder(orderFiles[b]);
    int64_t r = 0;
    int d = 0;
    urows[b] = readRows(unsFeatFiles[b], &r, &d);
    if (r > 0 && dim > 0 && d != dim) perr("Error: invalid data file dimension in " + unsFeatFiles[b]);
    if (r > 0) dim = d;
    if ((int64_t)(orders[b].size() / 3) != r)
      perr("Error: " + std::to_string(r) + " rows in " + unsFeatFiles[b] + " for " + std::to_string(orders[b].size() / 3) + " merges in " + orderFiles[b] + "...");
    blocks[b].rows = urows[b].data(); blocks[b].order = orders[b].data(); blocks[b].n_merges = r;
  }
#endif
  if (dim == 0) perr("Error: no rows in the feature files...");
  const int64_t n = (int64_t)(rows.size() / (size_t)dim);
  if ((int64_t)labels.size() != n) perr("Error: " + std::to_string(labels.size()) + " labels for " + std::to_string(n) + " rows...");
  std::vector<double> mn, mx, init;
  if (a.has("fmm")) {
    int64_t r = 0;
    int d = 0;
    const std::vector<double> t = readRows(a.str("fmm"), &r, &d);
    if (r < 2 || d < dim) perr("Error: the min/max file needs two rows of at least " + std::to_string(dim) + " values: " + a.str("fmm"));
    mn.assign(t.begin(), t.begin() + dim); mx.assign(t.begin() + d, t.begin() + d + dim);
  }
  if (a.has("im")) {
    if (verbose) printf("Initializing from input model...\n");
    int64_t nw = 0;
    check(glia_hmt_mlp_file_parse(a.str("im").c_str(), nullptr, 0, &nw));
    init.resize((size_t)nw);
    check(glia_hmt_mlp_file_parse(a.str("im").c_str(), init.data(), nw, &nw));
    const int64_t want = o.n1 > 0 ? (int64_t)(dim + 1) * o.n1 + (int64_t)(o.n1 + 1) * o.n2 + o.n2 + 1 : dim + 1;
    if (nw != want) perr("Error: the input model holds " + std::to_string(nw) + " weights, rows of " + std::to_string(dim) + " columns need " + std::to_string(want));
  }
  glia_hmt_ctx* ctx;
  check(glia_hmt_ctx_create(0, nullptr, &ctx));
  glia_hmt_mlp_model* model;
  const double *pmn = mn.empty() ? nullptr : mn.data(), *pmx = mx.empty() ? nullptr : mx.data(), *pinit = init.empty() ? nullptr : init.data();
#ifdef GLIA_TRAIN_SSHMT
  if (batches)
    check(glia_hmt_sshmt_train_batches(ctx, n ? rows.data() : nullptr, n, dim, n ? labels.data() : nullptr, blocks.data(), (int)blocks.size(), &so, &bo,
                                       pmn, pmx, pinit, &model));
  else
    check(glia_hmt_sshmt_train(ctx, n ? rows.data() : nullptr, n, dim, n ? labels.data() : nullptr, blocks.data(), (int)blocks.size(), &so, pmn, pmx,
                               pinit, &model));
#else
  if (batches) check(glia_hmt_mlp_train_batches(ctx, rows.data(), n, dim, labels.data(), &o, &bo, pmn, pmx, pinit, &model));
  else check(glia_hmt_mlp_train(ctx, rows.data(), n, dim, labels.data(), &o, pmn, pmx, pinit, &model));
#endif
  int rounds = 0, stopped = 0, nSigma = 0;
  int64_t nTrace = 0, used = 0, nPaths = 0, nUnsRows = 0;
  check(glia_hmt_mlp_model_info(model, &rounds, nullptr, &nTrace, &stopped, &used, &nSigma));
  check(glia_hmt_mlp_model_paths(model, &nPaths, &nUnsRows));
  if (verbose) {
    std::vector<glia_hmt_mlp_train_record> tr((size_t)nTrace);
    std::vector<double> s2((size_t)nSigma), s2e((size_t)nSigma), u2((size_t)nSigma), u2e((size_t)nSigma);      // (su: zeros without the term)
    check(glia_hmt_mlp_model_trace(model, tr.data()));
    check(glia_hmt_mlp_model_sigmas(model, s2.data(), s2e.data()));
    check(glia_hmt_mlp_model_sigmas_u(model, u2.data(), u2e.data()));
    printf("Use %lld supervised samples.\n", (long long)used);
#ifdef GLIA_TRAIN_SSHMT
    printf("Use %lld unsupervised samples.\n", (long long)nPaths);
#endif
    size_t k = 0;
    for (int i = 0; i < nSigma; ++i) {
      printf("\tlearn-%d: su = %g (%g), ss = %g (%g)\n", i, std::sqrt(u2[i]), std::sqrt(u2e[i]), std::sqrt(s2[i]), std::sqrt(s2e[i]));
      for (; k < tr.size() && tr[k].round == i; ++k)
        printf("\tgd: %-6d fx = %-12g |x| = %-12g |g| = %-12g step = %g\n", tr[k].t, tr[k].fx, tr[k].xnorm, tr[k].gnorm, tr[k].step);
    }
  }
  if (stopped) std::cerr << kTool << ": stopped in round " << rounds - 1 << ": the energy or its gradient is not finite; the weights from before that step are kept" << std::endl;
  for (int i = 0; i < rounds && o.n_sigma_updates > 0; ++i) {
    if (!((i + 1) % saveInterval == 0 || i == o.n_sigma_updates - 1 || (stopped && i == rounds - 1))) continue;
    char path[4096];
    snprintf(path, sizeof(path), pattern.c_str(), i);
    check(glia_hmt_mlp_model_write(model, path, i));
  }
  glia_hmt_mlp_model_free(model);
  glia_hmt_ctx_destroy(ctx);
  return EXIT_SUCCESS;
}
