// myosim_inverse.hip -- host side of libmyosim_inverse.so (include/myosim_inverse.h): model handle, argument checks, launch.
// The kernels are k_inverse<G, NVP, GEN> (myosim_inverse_kernel.hpp), instantiated in myosim_inverse_inst_*.hip.
#include <stddef.h>

#include <memory>
#include <string>

#include "myosim_inverse_kernel.hpp"
#include "../myosim_launch_plan.hpp"
#include "../../../include/myosim_inverse.h"

MM_KERNEL_LIST(MMI_DECLARE)

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define MM_HOST_FAIL fail
#include "../myosim_host.hpp"

struct mm_inverse_model : OnDevice<ModelImage> {};   // the compiled model (myosim_model_compile.hpp) + its device copy

extern "C" const char* mm_inverse_last_error(void) { return g_err.c_str(); }
extern "C" int mm_inverse_abi_version(void) { return MM_INVERSE_ABI_VERSION; }

extern "C" void mm_inverse_destroy(mm_inverse_model* m) { delete m; }

extern "C" int mm_inverse_create(const uint32_t* blob, int nwords, int lanes_per_env, mm_inverse_model** out) {
  if (!out) return fail(MM_EARG, "mm_inverse_create: out is NULL");
  *out = nullptr;
  std::unique_ptr<mm_inverse_model> m(new mm_inverse_model());
  // The inverse has no integrator.  The model is compiled as an Euler model, so that the kernel family, the padded width and the
  // LDS layout are those of a (lanes, nvp, general rows) combination of the Euler list -- the combinations k_inverse is built for --
  // whatever integrator the blob names.
  std::vector<uint32_t> euler;
  {
    mmc::BlobView b;
    if (int rc = mmc::open_blob(blob, nwords, b, g_err)) return rc;
    if (b.sec[MM_SEC_OPT_I] < 0 || b.sec[MM_SEC_OPT_I] + MM_OI_INTEGRATOR >= nwords) return fail(MM_EBADBLOB, "option section outside the blob");
    const int integ = (int)blob[b.sec[MM_SEC_OPT_I] + MM_OI_INTEGRATOR];
    if (integ != MM_INT_EULER && integ != MM_INT_RK4 && integ != MM_INT_IMPLICITFAST)
      return fail(MM_EUNSUPPORTED, "integrator must be Euler (0), RK4 (1) or implicitfast (3)");
    euler.assign(blob, blob + nwords);
    euler[b.sec[MM_SEC_OPT_I] + MM_OI_INTEGRATOR] = (uint32_t)MM_INT_EULER;
  }
  { const int rc = compile_model(euler.data(), nwords, *m, g_err); if (rc != MM_OK) return rc; }
  m->lanes_auto = 0;   // one width per handle (the model's default, or lanes_per_env below), whatever the batch size
  if (m->rpl != 1)
    return fail(MM_EUNSUPPORTED, "mm_inverse: models with njmax > 64 (the two-rows-per-lane kernel family) have no inverse kernel");
  if (lanes_per_env) {
    if (!check_lanes(m.get(), lanes_per_env) || !have_kernel(lanes_per_env, m->nvp, m->d.gen, 0, 1))
      return fail(MM_EARG, "lanes_per_env must be 4/8/16/32/64, >= nbody, nv, njnt, padded nv (and constraint rows), with a compiled kernel");
    m->lanes = lanes_per_env;
    build_layout(m.get());
    write_consts(m.get());
  }
  if (!have_kernel(m->lanes, m->nvp, m->d.gen, 0, 1)) return fail(MM_EUNSUPPORTED, "no compiled inverse kernel for this (lanes_per_env, nv) combination");
  if (int rc = upload_model(m.get())) return rc;
  *out = m.release();
  return MM_OK;
}

extern "C" int mm_inverse_info(const mm_inverse_model* m, int which) {
  if (!m) return MM_EARG;
  switch (which) {
    case MM_INVERSE_INFO_LANES: return m->lanes;
    case MM_INVERSE_INFO_KERNEL_FAMILY: return m->d.gen ? 2 : (m->nvp >= 8 ? 1 : 0);
    case MM_INVERSE_INFO_EFC_ROWS: return m->d.gen ? m->d.efc_rows : 0;
    case MM_INVERSE_INFO_NVP: return m->nvp;
    case MM_INVERSE_INFO_NV: return m->d.nv;
    case MM_INVERSE_INFO_NU: return m->d.nu;
    case MM_INVERSE_INFO_NQ: return m->d.nq;
    case MM_INVERSE_INFO_LDS_BYTES_PER_ENV: return (int)m->lds_per_env;
    case MM_INVERSE_INFO_ARGS_SIZE: return (int)sizeof(mm_inverse_args);
  }
  return MM_EARG;
}

// the planner's geometry with the model read through L2 and no helper waves (k_inverse has neither form)
static int launch_on_device(const mm_inverse_model* m, KArgs& a, const InvArgs& v, void* stream) {
  LaunchOptions opt;
  opt.lds_model = 0;
  LaunchPlan p;
  if (int rc = plan_launch(*m, opt, 0, a.s.nenv, false, p, g_err)) return rc;
  const void* fn = nullptr;
#define X0(G_, N_, GN_) if (p.lanes == G_ && m->nvp == N_ && m->d.gen == GN_) fn = (const void*)k_inverse<G_, N_, GN_ != 0>;
#define X1(G_, N_, GN_)
#define X2(G_, N_, GN_)
#define X(G_, N_, GN_, RK_) X##RK_(G_, N_, GN_)
  MM_KERNEL_LIST(X)
#undef X
#undef X0
#undef X1
#undef X2
  if (!fn) return fail(MM_EUNSUPPORTED, "no compiled inverse kernel for this (lanes_per_env, nv) combination");
  // the dynamic-LDS limit is a per-device attribute of the function (set on every launch: the call is cheap next to the kernel)
  HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  void* args[] = {&a, const_cast<InvArgs*>(&v)};
  (void)hipLaunchKernel(fn, dim3(p.blocks), dim3(p.threads), args, p.lds_bytes, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MM_OK;
}

extern "C" int mm_inverse(const mm_inverse_model* m, const mm_state* s, const float* qacc, const mm_inverse_args* args, void* stream) {
  if (!m || !s || !qacc || !args) return fail(MM_EARG, "mm_inverse: NULL model, state, qacc or args");
  if (s->nenv < 1) return fail(MM_EARG, "mm_inverse: nenv < 1");
  const size_t min_size = offsetof(mm_inverse_args, qfrc_inverse) + sizeof(float*);
  if (args->size > sizeof(mm_inverse_args))
    return fail(MM_EARG, "mm_inverse_args.size is larger than this library's struct: the caller was built against a newer header");
  if (args->size < min_size) return fail(MM_EARG, "mm_inverse_args.size is smaller than the struct's required head (size, constraints, qfrc_inverse)");
  mm_inverse_args p;
  memset(&p, 0, sizeof(p));
  memcpy(&p, args, args->size);
  if (!p.qfrc_inverse) return fail(MM_EARG, "mm_inverse: qfrc_inverse is NULL (the one required output)");
  if (!s->qpos || !s->qvel) return fail(MM_EARG, "mm_inverse: mm_state.qpos / qvel is NULL");
  // per-env model deltas are refused, never ignored
  if (s->geom_size_env || s->geom_type_env || s->body_mass_env || s->body_pos_env)
    return fail(MM_EUNSUPPORTED, "mm_inverse: the state carries a per-env model delta (geom_size_env / geom_type_env / body_mass_env / body_pos_env), which the inverse does not implement");
  KArgs a;
  fill_kargs(a, m, s);
  a.mode = 1;
  InvArgs v;
  memset(&v, 0, sizeof(v));
  v.qacc = qacc; v.constraints = p.constraints ? 1 : 0;
  v.qfrc_inverse = p.qfrc_inverse; v.qfrc_mass = p.qfrc_mass; v.qfrc_bias = p.qfrc_bias; v.qfrc_passive = p.qfrc_passive;
  v.qfrc_constraint = p.qfrc_constraint; v.nefc = p.nefc; v.actuator_moment = p.actuator_moment; v.actuator_gain = p.actuator_gain;
  v.actuator_bias = p.actuator_bias; v.actuator_length = p.actuator_length; v.actuator_velocity = p.actuator_velocity;
  DeviceGuard guard(m->device);
  if (guard.err != hipSuccess) return fail(MM_EHIP, guard.message());
  return launch_on_device(m, a, v, stream);
}
