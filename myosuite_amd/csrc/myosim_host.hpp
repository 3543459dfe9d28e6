#pragma once
// myosim_host.hpp -- the host plumbing shared by myosim_engine.hip, inverse/myosim_inverse.hip and myosim_ppo.hip: the check of a
// HIP call, the switch to a handle's device, the device copy of a compiled model and the kernel arguments every model kernel takes.
// Each includer keeps its own thread-local error string (mm_last_error, mm_inverse_last_error and mm_ppo_last_error are distinct)
// and names the function that sets it before the include:
//     #define MM_HOST_FAIL fail        // int fail(int code, const std::string& msg)
#include <hip/hip_runtime.h>
#include <string.h>
#include <string>

#define HIPCHK(x)                                                                                         \
  do {                                                                                                    \
    hipError_t e_ = (x);                                                                                  \
    if (e_ != hipSuccess) return MM_HOST_FAIL(MM_EHIP, std::string(#x) + ": " + hipGetErrorString(e_));   \
  } while (0)

// The launches of a handle go to ITS device (the caller's stream must belong to it), whatever device is current in the calling
// thread; the caller's current device is restored on scope exit.  `err` is the failure of the switch, message() its text.
struct DeviceGuard {
  int prev = -1;   // device to go back to (-1: none)
  hipError_t err = hipSuccess;
  const char* call = "";
  explicit DeviceGuard(int dev, const char* set_call = "hipSetDevice(m->device)") {
    int cur = -1;
    if ((err = hipGetDevice(&cur)) != hipSuccess) { call = "hipGetDevice(&cur)"; return; }
    if (cur == dev) return;
    if ((err = hipSetDevice(dev)) != hipSuccess) { call = set_call; return; }
    prev = cur;
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
  std::string message() const { return std::string(call) + ": " + hipGetErrorString(err); }
};

// a compiled model (ModelImage, myosim_model_compile.hpp) and the device copy of its words, on the device current at upload
template <class Image>
struct OnDevice : Image {
  uint32_t* d_blob = nullptr;
  int device = 0;
  ~OnDevice() { if (d_blob) (void)hipFree(d_blob); }
};
template <class Model>
static int upload_model(Model* m) {
  HIPCHK(hipGetDevice(&m->device));
  HIPCHK(hipMalloc((void**)&m->d_blob, m->words.size() * sizeof(uint32_t)));
  HIPCHK(hipMemcpy(m->d_blob, m->words.data(), m->words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  return MM_OK;
}

// KArgs of a launch of model `m` on state `s`: the image's tables and the state, per-env model deltas that name nothing dropped
template <class Args, class Model, class State>
static void fill_kargs(Args& a, const Model* m, const State* s) {
  memset(&a, 0, sizeof(a));
  a.blob = m->d_blob; a.cofs = m->cofs; a.blob_words = m->blob_words;
  memcpy(a.sec, m->sec, sizeof(a.sec));
  a.d = m->d; a.L = m->L; a.D = m->D; a.x = m->x; a.s = *s;
  if (!a.s.geom_size_env || a.s.geom_env_id < 0 || a.s.geom_env_id >= m->d.ngeom) { a.s.geom_size_env = nullptr; a.s.geom_type_env = nullptr; a.s.geom_env_id = -1; }
  if (!a.s.body_mass_env || a.s.body_mass_env_id <= 0 || a.s.body_mass_env_id >= m->d.nbody) { a.s.body_mass_env = nullptr; a.s.body_mass_env_id = -1; }
  if (!a.s.body_pos_env || a.s.body_pos_env_id <= 0 || a.s.body_pos_env_id >= m->d.nbody) { a.s.body_pos_env = nullptr; a.s.body_pos_env_id = -1; }
}
