// kernel_choice_main.cpp -- which compiled kernel a model runs on, from the host-only model compiler and launch planner
// (myosuite_amd/csrc/myosim_model_compile.hpp, myosim_launch_plan.hpp) as a plain host program, for the host sanitizers
// (tests/test_wide_models.py):
//   kernel_choice_main BLOB [LANES [PRECISION [NENV]]]   compile_model on the blob, then set_lanes (LANES > 0) and set_option
//       "precision" (PRECISION > 0) as mm_model_create's callers do, and one line on stdout: "code lanes nvp gen integ_kernel rpl" --
//       code is the first refusal (then a second line holds its message), the rest names the k_engine<lanes, nvp, gen, integ_kernel>
//       (rpl = 2: k_engine_rows2<nvp>) instantiation of myosim_inst_list.hpp that a launch over NENV envs (default 1) runs: lanes
//       is the planner's pick_lanes(), which for an unpinned limit-rows-only model depends on the batch size, not the model's
//       default width.
#include <stdio.h>
#include <stdlib.h>

#include "../../myosuite_amd/csrc/myosim_launch_plan.hpp"

int main(int argc, char** argv) {
  if (argc < 2 || argc > 5) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  std::vector<uint32_t> blob;
  for (uint32_t w; fread(&w, 4, 1, in) == 1;) blob.push_back(w);
  fclose(in);
  const int lanes = argc > 2 ? atoi(argv[2]) : 0, precision = argc > 3 ? atoi(argv[3]) : 0, nenv = argc > 4 ? atoi(argv[4]) : 1;
  ModelImage m{};
  LaunchOptions opt;
  std::string err;
  int rc = compile_model(blob.data(), (int)blob.size(), m, err);
  if (rc == MM_OK && lanes > 0) rc = set_lanes(&m, &opt, lanes, err);
  if (rc == MM_OK && precision > 0) {
    bool consts = false;
    rc = set_option(&m, &opt, "precision", precision, consts, err);
  }
  if (rc == MM_OK) write_consts(&m);
  printf("%d %d %d %d %d %d\n", rc, rc == MM_OK ? pick_lanes(&m, nenv) : m.lanes, m.nvp, m.d.gen, integ_kernel(m.d.integrator), m.rpl);
  if (rc != MM_OK) printf("%s\n", err.c_str());
  return 0;
}
