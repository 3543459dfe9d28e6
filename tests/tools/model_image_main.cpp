// model_image_main.cpp -- the model compiler (myosuite_amd/csrc/myosim_model_compile.hpp) as a plain host program, for the host
// sanitizers: model_image_main BLOB OUT reads a model blob and writes the ModelImage as a flat file (tests/test_model_image.py):
// 16 int32 {code, lanes, lanes_auto, nvp, rpl, nseg, nwrapitem, nfolded, blob_words, cofs, cofs_tw, lds_per_env, lds_per_env_tw,
// image words, 0, 0}, then the refusal message, or DbgLayout, origin[3] and the image words.
#include <stdio.h>

#include "../../myosuite_amd/csrc/myosim_model_compile.hpp"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  std::vector<uint32_t> blob;
  for (uint32_t w; fread(&w, 4, 1, in) == 1;) blob.push_back(w);
  fclose(in);
  ModelImage m{};
  std::string err;
  const int rc = compile_model(blob.data(), (int)blob.size(), m, err);
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  const int32_t head[16] = {rc, m.lanes, m.lanes_auto, m.nvp, m.rpl, m.nseg, m.nwrapitem, m.nfolded, m.blob_words, m.cofs, m.cofs_tw,
                            (int32_t)m.lds_per_env, (int32_t)m.lds_per_env_tw, (int32_t)m.words.size(), 0, 0};
  fwrite(head, 4, 16, out);
  if (rc != MM_OK) fwrite(err.data(), 1, err.size(), out);
  else {
    fwrite(&m.D, sizeof(m.D), 1, out);
    fwrite(m.origin, 4, 3, out);
    fwrite(m.words.data(), 4, m.words.size(), out);
  }
  return fclose(out) == 0 ? 0 : 2;
}
