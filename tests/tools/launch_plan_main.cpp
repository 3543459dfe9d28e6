// launch_plan_main.cpp -- the launch planner (myosuite_amd/csrc/myosim_launch_plan.hpp, on myosim_model_compile.hpp) as a plain host
// program, for the host sanitizers (tests/test_launch_plan.py):
//   launch_plan_main model BLOB SCRIPT OUT   compiles the blob ("create CODE") and runs the script's lines in order:
//       lanes N             set_lanes         -> "call CODE MESSAGE"
//       option NAME VALUE   set_option        -> "call CODE MESSAGE"
//       plan NENV OBS       plan_launch       -> "plan CODE lanes waves two_wave lds_model lds_bytes blocks"
//                                                (waves = threads / 64, helper waves included: MM_LAUNCH_WAVES_PER_BLOCK)
//   launch_plan_main inverse SCRIPT OUT      the planner as the inverse library calls it (lds_model = 0, helper waves off), for every
//       Euler (lanes, nvp, general rows) of MM_KERNEL_LIST, four per-env table sizes and three batch sizes:
//       "inverse lanes nvp gen per_env nenv CODE lanes waves two_wave lds_model lds_bytes blocks threads"
#include <stdio.h>

#include "../../myosuite_amd/csrc/myosim_launch_plan.hpp"

static void print_plan(FILE* out, int rc, const LaunchPlan& p, bool threads) {
  fprintf(out, "%d %d %d %d %d %zu %d", rc, p.lanes, threads ? p.waves_per_block : p.threads / 64, p.two_wave, p.lds_model, p.lds_bytes, p.blocks);
  if (threads) fprintf(out, " %d", p.threads);
  fprintf(out, "\n");
}

static int run_model(const char* blob_path, FILE* in, FILE* out) {
  FILE* bf = fopen(blob_path, "rb");
  if (!bf) return 2;
  std::vector<uint32_t> blob;
  for (uint32_t w; fread(&w, 4, 1, bf) == 1;) blob.push_back(w);
  fclose(bf);
  ModelImage m{};
  LaunchOptions opt;
  std::string err;
  const int rc = compile_model(blob.data(), (int)blob.size(), m, err);
  fprintf(out, "create %d\n", rc);
  if (rc != MM_OK) return 0;
  char cmd[32], name[64];
  while (fscanf(in, "%31s", cmd) == 1) {
    int a = 0, b = 0;
    if (!strcmp(cmd, "lanes") && fscanf(in, "%d", &a) == 1) {
      err.clear();
      const int r = set_lanes(&m, &opt, a, err);
      if (r == MM_OK) write_consts(&m);
      fprintf(out, "call %d %s\n", r, err.c_str());
    } else if (!strcmp(cmd, "option") && fscanf(in, "%63s %d", name, &a) == 2) {
      err.clear();
      bool consts = false;
      const int r = set_option(&m, &opt, name, a, consts, err);
      if (r == MM_OK && consts) write_consts(&m);
      fprintf(out, "call %d %s\n", r, err.c_str());
    } else if (!strcmp(cmd, "plan") && fscanf(in, "%d %d", &a, &b) == 2) {
      LaunchPlan p{};
      const int r = plan_launch(m, opt, 1, a, b != 0, p, err);
      fprintf(out, "plan ");
      print_plan(out, r, p, false);
    } else return 2;
  }
  return 0;
}

static void run_inverse(FILE* out) {
  LaunchOptions opt;
  opt.lds_model = 0;
#define X(G_, N_, GN_, RK_)                                                                          \
  if (RK_ == 0)                                                                                      \
    for (size_t per_env : {(size_t)1024, (size_t)24 * 1024, (size_t)60 * 1024, (size_t)170 * 1024})  \
      for (int nenv : {1, 4096, 200000}) {                                                           \
        ModelImage m{};                                                                              \
        m.lanes = G_; m.lanes_auto = 0; m.nvp = N_; m.d.gen = GN_; m.d.integrator = MM_INT_EULER;    \
        m.lds_per_env = per_env; m.lds_per_env_tw = 2 * per_env; m.blob_words = 5000;                \
        LaunchPlan p{};                                                                              \
        std::string err;                                                                             \
        const int rc = plan_launch(m, opt, 0, nenv, false, p, err);                                  \
        fprintf(out, "inverse %d %d %d %zu %d ", G_, N_, GN_, per_env, nenv);                        \
        print_plan(out, rc, p, true);                                                                \
      }
  MM_KERNEL_LIST(X)
#undef X
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const bool model = !strcmp(argv[1], "model");
  if (model ? argc != 5 : (strcmp(argv[1], "inverse") || argc != 4)) return 2;
  FILE* in = fopen(argv[argc - 2], "r");
  FILE* out = fopen(argv[argc - 1], "w");
  if (!in || !out) return 2;
  int rc = 0;
  if (model) rc = run_model(argv[2], in, out);
  else run_inverse(out);
  fclose(in);
  return fclose(out) == 0 ? rc : 2;
}
