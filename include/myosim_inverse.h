/* myosim_inverse.h -- C ABI of libmyosim_inverse.so: batched inverse dynamics (MuJoCo's mj_inverse) on gfx950.
 *
 * Given (qpos, qvel) of every env and an acceleration qacc, one launch returns the generalised force that produces it:
 *
 *     qfrc_inverse = M qacc + qfrc_bias - qfrc_passive - qfrc_constraint
 *
 * The envs are independent, so the frames of a trajectory are a batch (myosuite_amd/inverse.py: inverse_dynamics_trajectory).
 * The library is separate from libmyosim_hip.so and shares no handle with it: a model is compiled from the same blob
 * (include/myosim_model.h) by mm_inverse_create.  mm_state and the MM_* status codes are those of include/myosim.h; the state rows
 * are read-only here (qpos and qvel are read, nothing is written), and the model's integrator is ignored.
 *
 * Refused with MM_EUNSUPPORTED (mm_inverse_last_error() names the reason): models with njmax > 64, fp64, and a state that carries a
 * per-env model delta (geom_size_env / geom_type_env / body_mass_env / body_pos_env). */
#ifndef MYOSIM_INVERSE_H
#define MYOSIM_INVERSE_H
#include <stdint.h>

#include "myosim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MM_INVERSE_ABI_VERSION 1

typedef struct mm_inverse_model mm_inverse_model;

/* lanes_per_env: 0 = the narrowest group width that owns the model; else 4 / 8 / 16 / 32 / 64 with a compiled kernel (MM_EARG) */
int  mm_inverse_create(const uint32_t* blob, int nwords, int lanes_per_env, mm_inverse_model** out);
void mm_inverse_destroy(mm_inverse_model*);
const char* mm_inverse_last_error(void);
int  mm_inverse_abi_version(void);

enum { MM_INVERSE_INFO_LANES = 0,       /* lanes per env of the launch */
       MM_INVERSE_INFO_KERNEL_FAMILY,   /* as MM_INFO_KERNEL_FAMILY: 0 limit rows, dense (nv <= 4); 1 limit rows, tree-sparse M; 2 general rows */
       MM_INVERSE_INFO_EFC_ROWS,        /* constraint rows allocated per env by the general-row kernels (0: limit rows only) */
       MM_INVERSE_INFO_NVP,             /* padded nv of the kernel */
       MM_INVERSE_INFO_NV, MM_INVERSE_INFO_NU, MM_INVERSE_INFO_NQ,
       MM_INVERSE_INFO_LDS_BYTES_PER_ENV,
       MM_INVERSE_INFO_ARGS_SIZE };     /* sizeof(mm_inverse_args) in the library's build */
int  mm_inverse_info(const mm_inverse_model*, int which);   /* MM_EARG for an unknown `which` */

typedef struct {
  uint32_t size;              /* sizeof(mm_inverse_args) in the caller's build: fields are only ever appended; the library copies
                                 min(size, its own sizeof) bytes and zero-fills the rest, and refuses a larger size (MM_EARG) */
  int    constraints;         /* 0: constraint forces disabled (mjDSBL_CONSTRAINT, as the reference's inverse-dynamics tutorial);
                                 1: mj_invConstraint -- the row law of the forward solve evaluated at qacc */
  float* qfrc_inverse;        /* [nenv][nv] required */
  float *qfrc_mass, *qfrc_bias, *qfrc_passive, *qfrc_constraint;   /* [nenv][nv] optional (NULL = not requested) */
  int32_t* nefc;              /* [nenv] optional: constraint rows of the env (0 with constraints = 0) */
  float* actuator_moment;     /* [nenv][nu][nv] optional, dense */
  float *actuator_gain, *actuator_bias, *actuator_length, *actuator_velocity;   /* [nenv][nu] optional: actuator_force = gain * act + bias
                                                                                   (before any force range) */
} mm_inverse_args;

/* One launch on the handle's device and the caller's stream.  MM_EARG: NULL handle / state / qacc / args / qfrc_inverse, nenv < 1, a
 * `size` beyond the library's.  Nothing is written when a call is refused. */
int  mm_inverse(const mm_inverse_model*, const mm_state* s, const float* qacc, const mm_inverse_args*, void* stream);

#ifdef __cplusplus
}
#endif
#endif
