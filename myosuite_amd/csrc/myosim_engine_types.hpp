#pragma once
// myosim_engine_types.hpp -- the plain structs shared by the kernels and the host-only model compiler (myosim_model_compile.hpp).
// No HIP here: this header also compiles with a plain host C++ compiler.
#include <stdint.h>

#include "../../include/myosim_model.h"
#include "../../include/myosim.h"

struct Dims {
  int nq, nv, nu, na, nbody, njnt, ngeom, nsite, ntendon, nwrap, neq, npair, nM, nlevel, njmax, ntenJ;
  int iterations, ls_iterations, eulerdamp, any_damping;
  int gen;   // model has equality / friction-loss / contact rows: general (dense-J) constraint path
  int nfric; // dofs with frictionloss > 0 (one friction-loss row each, behind the equalities)
  int ntlim; // limited tendons (at most one limit row each, behind the joint-limit rows)
  int dof_nlevel;   // levels of the dof tree (1 + maximum number of ancestor dofs)
  // SP kernels: the dof tree cut into segments (maximal unbranched chains); one lane eliminates a whole segment
  int bchain_nlevel;    // body chains (Engine::subtree_sum): levels of the chain tree | most child chains << 4 | longest chain << 8; 0: the host could not build the chains
  int seg_nlevel;       // levels of the segment tree
  int seg_lvinfo[2];    // one byte per segment level: [3:0] most child segments of a segment there
  int seg_lvtb[2];      // one byte per segment level: [3:0] top depth, [7:4] bottom depth of the segments there (all alike)
  int seg_zero;         // index of the all-zero update-matrix slot (absent children)
  int seg_u;            // word offset (in the u1 LDS region) of the update matrices, 36 words per segment
  int desc_words;       // words of the per-dof descendant list (4 ids each) a product M x has to walk
  int integrator;   // MM_INT_EULER | MM_INT_RK4 | MM_INT_IMPLICITFAST
  int efc_rows;     // allocated rows of the efc_J LDS table: min(lanes_per_env, njmax rounded up to 4)
  int condim4;      // 1: some contact pair is condim 4 (torsional friction: six pyramid rows) -- the torsional pass runs
  int nconmax;      // MM_OI_NCONMAX: contacts beyond this many (in collider order) are dropped and flagged, as mjModel.nconmax
  float timestep, gx, gy, gz, tolerance, ls_tolerance, meaninertia;
  // Origin of the kernel's internal world frame (host: mean body position at qpos0, rounded to 1/64 m).  Physics is
  // translation invariant; fp32 rounding is not: a hand that sits 1 m from the world origin carries ~1e-7 m of absolute
  // error in every point, i.e. ~2e-5 of a 5 mm tendon moment arm.  All positions inside the kernel are relative to this
  // origin; qpos of free joints, task targets and every position OUTPUT stay in world coordinates.
  float ox, oy, oz;
};

// per-env LDS tables (offsets in 32-bit words from the env's base)
struct Layout {
  int qpos, qvel, act, ctrl, actdot;
  int xpos, xmat, xanchor, xaxis, com, cdof;
  int u1;   // union: xquat[4nb] during FK | (cvel,cacc)[12nb] then cfrc[6nb] during the velocity stage | dense NVP*NVP tile afterwards
  int crb;
  int tenlen, tenvel, tenj, tenfrc, actlen, actvel, actfrc;
  int mtile;   // two-wave launches: a second dense NVP x NVP tile (M for the helper wave, which leaves Euler's factor in it) + NVP words (1 / diagonal)
  int flags;   // two-wave launches: [0] passes the main wave has opened (kinematics done), [1] passes the helper wave has finished
  int wrapw;   // per wrapping path item: the two tangent points and a wrapped flag (7 words); inside u1 (free between FK and the velocity stage) when it fits
  int vec;  // nv: joint-transmission actuator forces
  int xvec; // NVP (16-byte aligned): operand vector of M x products routed through LDS
  int rk_qpos0, rk_act0, rk_adot;   // RK4: state at the start of the step, weighted act_dot sum (RK4 models only)
  int tenw, dofw;   // implicitfast: velocity-derivative weights per tendon (b_t - sum_a s_a gear_a^2) and per dof (damping - joint actuators)
  int efcJ, rowtab;   // general constraint rows: J [G][NVP+4] (16-byte aligned rows), row table [G][3] (GEN models only)
  int total;
};

#ifndef MM_FOLD_RIGID_SEGMENTS
#define MM_FOLD_RIGID_SEGMENTS 1   /* 0: every site-site segment of a tendon path is a path item of the kernel's sweep (rounds 1-5) --
                                      the reference path of paired accuracy comparisons */
#endif
// debug dump layout (tests only): one record per env in global memory
struct DbgLayout {
  int xpos, xquat, xipos, cdof, cvel, tenlen, tenvel, tenj, actfrc, actdot, M, bias, smooth, qaccsm, qacc, qfrccon,
      efc_active, efc_D, efc_aref, scal, total;
};

// engine-private tables appended behind the model blob on the device
struct Aux {
  int body_depth, body_rootslot, dof_rootslot;
  int root_list, nroot;
  int jent, jrec;        // tendon Jacobian by entry: jent [ntenJ], one word per entry in processing order: first row | rows << 24; rows (jrec) [..][4] (host: tendon_jacobian_rows)
  int item_tab, nitem;   // flattened tendon path items (4 words each), wraps first: see tendon()
  int dof_rel;           // per dof: 64-bit mask (2 words) of the dofs on its kinematic chain (ancestors, descendants, itself)
  int body_dofmask;      // per body: 64-bit mask (2 words) of the dofs between the body and the root of its tree (its chain)
  int dof_desc;          // per dof: ids of all its descendants, one byte each, 0xff-padded to 8 words
  int dof_seg;           // per dof, 6 words: segment owned by the dof's lane (the segment's top dof) or -1; path and child bytes; the dof's depth
  int dof_anc;           // per dof, 2 words: ids of its ancestor dofs by depth, one byte each
  int jnt_pack;          // per joint, 2 words: type | dofadr << 4 | qposadr << 14, bits(qpos0[qposadr]) -- one load instead of type -> address -> qpos0
  int body_chain;        // per body, 3 words: chain owned by the body's lane (its top body): bottom | level << 8 | children << 12, or -1; child chain tops, one byte each
  int ten_len0, ten_len0_f64;   // per tendon: the summed length of its path segments between rigidly connected bodies (folded at create): float table, double table
};

// model constants the kernel reads through the scalar cache (appended to the device blob at KArgs::cofs, see KD / KL / KX)
struct ConstBlock { Dims d; Layout L; Aux x; };
