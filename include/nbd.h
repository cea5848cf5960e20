/* nbd.h -- C-ABI of libnbd_hip.so: the MI355X (gfx950) hot path of bikuta6/nbody-deep-sim.
 *
 * The reference is pure Python and has no FFI layer of its own; its boundary for this path is
 * the Python API (src/galaxify/simulation.py, gnn.py, contconv.py, trainer.py). Each entry
 * point below names the reference lines whose arithmetic it replaces. The Python host classes
 * in nbody-deep-sim_amd/ keep the reference's names/arguments and call these through ctypes
 * (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - every pointer is a caller-owned DEVICE pointer (HBM) unless it says "host";
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls are asynchronous;
 *   - return 0 on success, a positive hipError_t if the HIP runtime failed, a negative
 *     NBD_E_* for argument errors; nothing throws, nothing allocates, no global mutable state;
 *   - all arithmetic is IEEE fp32 ("f32" suffix), indices are int32 on the ABI and int64 where
 *     the reference's tensors are int64 (edge_index).
 */
#ifndef NBD_H_
#define NBD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NBD_ABI_VERSION 2
#define NBD_E_BADARG (-1)   /* null pointer / negative size / misaligned buffer              */
#define NBD_E_WORKSPACE (-2) /* workspace smaller than nbd_*_workspace_bytes() reported        */
#define NBD_E_UNSUPPORTED (-3)

#define NBD_SRC_PAD 64      /* packed source arrays are padded to a multiple of this          */
#define NBD_CC_TILE 128     /* nodes per tile of the fused ContinuousConv kernels             */
#define NBD_CC_GROUPS 8     /* cell groups of the fused ContinuousConv kernel (one per XCD)     */
#define NBD_CC_MAX_RES 4    /* filter resolutions per nbd_contconv_pairs_batch_f32 call       */

typedef void* nbd_stream_t;

int nbd_abi_version(void);
/* sizeof() of the argument structs below as this library was compiled, by name ("nbd_gnn_layer_args", ...; 0 for an
 * unknown name): a binding that mirrors a struct field for field checks its own size against this before the first call
 * (nbd/_lib.py does; tests/test_cabi.py holds every mirror to it). */
size_t nbd_struct_size(const char* name);
/* Human-readable text for a return code (static storage). */
const char* nbd_strerror(int code);

/* ---------------------------------------------------------------- direct-force integrator */

/* Length (in float4 entries) of the packed {x,y,z,m} array for n bodies: n rounded up to
 * NBD_SRC_PAD. Padding entries carry m = 0 and contribute exactly 0. */
int nbd_posm_padded_len(int n);

/* Pack positions (n,3) row-major + masses (n,) into float4 {x,y,z,m}[nbd_posm_padded_len(n)].
 * Layout step for nbd_accel_f32; replaces the implicit (N,3)/(N,) tensor reads of
 * simulation.py:80,87. posm must be 16-byte aligned. */
int nbd_pack_posm_f32(const float* pos, const float* mass, int n, float* posm, nbd_stream_t stream);

/* Bytes of scratch nbd_accel_f32 needs for this problem size (partial-force slabs). */
size_t nbd_accel_workspace_bytes(int n_src, int n_tgt);

/* Launch geometry nbd_accel_f32 will use (introspection for tests / bench / DESIGN.md):
 * groups = 128-target workgroup columns, slabs = source splits across workgroups,
 * chunks_per_wave = 64-source chunks each wave streams. Any out pointer may be NULL (host). */
int nbd_accel_plan(int n_src, int n_tgt, int* groups, int* slabs, int* chunks_per_wave);

/* All-pairs softened gravity, BaseSimulator.compute_accelerations (simulation.py:71-89):
 *   acc[i] = g_const * sum_j m_j (r_j - r_i) (|r_j - r_i|^2 + softening_sq)^(-3/2),
 * the pair with global index j == tgt_global_offset + i excluded (fill_diagonal_(0), :85).
 *   posm_src  packed sources, n_src real entries, nbd_posm_padded_len(n_src) allocated
 *   posm_tgt  packed targets (n_tgt entries; may point into posm_src)
 *   tgt_global_offset  index in the source numbering of target 0 (range partition, multi-GPU)
 *   softening_sq       (float)(softening**2), the fp32 scalar of simulation.py:82
 *   acc_out   (n_tgt,3) row-major fp32
 * Deterministic: same inputs give bit-identical outputs on every call. */
int nbd_accel_f32(const float* posm_src, int n_src, const float* posm_tgt, int n_tgt,
                  int tgt_global_offset, float softening_sq, float g_const, float* acc_out,
                  void* workspace, size_t workspace_bytes, nbd_stream_t stream);

/* Tuning hook: nbd_accel_f32 with an explicit launch geometry (slabs = source splits across workgroups,
 * 1..64; variant 0 = eight sources in flight per wave, 5 waves/SIMD; variant 1 = four, 8 waves/SIMD) and an
 * optional excluded source range [exclude_lo, exclude_hi) (those sources contribute nothing). The launch
 * plan of the library was chosen with it (tools/sweep_accel_plan.py); every geometry computes the same sums
 * in a different association, so results agree to rounding. Workspace: slabs * n_tgt * 3 floats. */
size_t nbd_accel_tuned_workspace_bytes(int n_tgt, int slabs);
int nbd_accel_tuned_f32(const float* posm_src, int n_src, int exclude_lo, int exclude_hi, const float* posm_tgt,
                        int n_tgt, int tgt_global_offset, float softening_sq, float g_const, float* acc_out,
                        void* workspace, size_t workspace_bytes, int slabs, int variant, nbd_stream_t stream);

/* ---- range-sharded step: one rank of a range partition owns bodies [lo, lo + n_local) of n_total
 * (the reference has no distributed code -- this is the same LeapFrogSimulator.step,
 * simulation.py:153-170, with the force sum of :80-88 split by source ownership). Per step and rank:
 *   nbd_kick_drift_f32(local state) -> posm_local
 *   [all-gather of posm_local into posm_all: issued by the host, asynchronous]
 *   nbd_shard_force_local_f32        own bodies as sources; runs while the gather is in flight
 *   [wait for the gather]
 *   nbd_shard_force_remote_f32       all other bodies as sources, then acc = G * (fixed-order sum of every
 *                                    partial-force slab of both launches) and v += c_kick * acc fused
 * posm_local: float4[nbd_posm_padded_len(n_local)] (padding zero); posm_all: float4[padded(n_total)] in
 * global order. Any lo / n_local is accepted (chunks of posm_all that straddle lo or lo + n_local are
 * walked with an element mask). vel may be NULL (no kick: compute_accelerations / Euler). Workspace as
 * nbd_shard_workspace_bytes, the same buffer for both calls of a step. Deterministic. */
int nbd_shard_plan(int n_total, int lo, int n_local, int* slabs_local, int* chunks_per_wave_local,
                   int* slabs_remote, int* chunks_per_wave_remote);
size_t nbd_shard_workspace_bytes(int n_total, int lo, int n_local);
int nbd_shard_force_local_f32(const float* posm_local, int n_local, float softening_sq, void* workspace,
                              size_t workspace_bytes, int n_total, int lo, nbd_stream_t stream);
int nbd_shard_force_remote_f32(const float* posm_all, int n_total, const float* posm_local, int n_local, int lo,
                               float softening_sq, float g_const, float* acc_out, float* vel, float c_kick,
                               void* workspace, size_t workspace_bytes, nbd_stream_t stream);
/* The same two launches for a system of EQUAL masses (see nbd_leapfrog_step_uniform_f32): the force kernels without their
 * per-pair mass multiply, g_const * mass_value applied once by the finishing pass. The caller vouches that every body's
 * mass equals mass_value. */
int nbd_shard_force_local_uniform_f32(const float* posm_local, int n_local, float softening_sq, void* workspace,
                                      size_t workspace_bytes, int n_total, int lo, nbd_stream_t stream);
int nbd_shard_force_remote_uniform_f32(const float* posm_all, int n_total, const float* posm_local, int n_local, int lo,
                                       float softening_sq, float g_const, float mass_value, float* acc_out, float* vel,
                                       float c_kick, void* workspace, size_t workspace_bytes, nbd_stream_t stream);

/* v += c_kick * a ; x += c_drift * v ; posm = pack(x, m)   (in place on pos, vel)
 * LeapFrogSimulator.step first half, simulation.py:164,166 with c_kick = (float)(0.5*dt),
 * c_drift = (float)dt; two roundings per update (mul then add), as torch eager does.
 * posm may be NULL (no packing). */
int nbd_kick_drift_f32(float* pos, float* vel, const float* acc, const float* mass, int n,
                       float c_kick, float c_drift, float* posm, nbd_stream_t stream);

/* v += c * a   (simulation.py:170, and :185 for Euler). */
int nbd_kick_f32(float* vel, const float* acc, int n, float c, nbd_stream_t stream);

/* x += c * v   (simulation.py:187). */
int nbd_drift_f32(float* pos, const float* vel, int n, float c, nbd_stream_t stream);

/* out[0..3n) = pos, out[3n..6n) = vel, out[6n..9n) = acc: the per-step state clones of BaseSimulator.run
 * (simulation.py:135-139) as one launch, so that a chunk of steps can be captured into a hipGraph with its
 * snapshots going to a device ring (one device->host copy per chunk instead of three per step). */
int nbd_snapshot_f32(const float* pos, const float* vel, const float* acc, int n, float* out, nbd_stream_t stream);
/* The same launch for a float64 state (the double-precision Hermite simulators): out is double[9n], 8-byte aligned. */
int nbd_snapshot_f64(const double* pos, const double* vel, const double* acc, int n, double* out, nbd_stream_t stream);

/* Bytes of scratch the fused step entry points need (always >= one slab). */
size_t nbd_step_workspace_bytes(int n);

/* Bytes of scratch at which the fused step runs its preferred plan; >= nbd_step_workspace_bytes(n), and equal to it
 * wherever the step does not take the symmetric force. The symmetric force keeps one partial-sum slot of n rows per
 * round of its tile tournament when the workspace holds them (K = min(M, 64) slots for M = 2 floor(n / 2048) tiles, one
 * more for the rows behind the last whole tile): every round then stores and all M (M - 1) / 2 tile pairs go in ONE
 * launch. A step entry reads the plan off workspace_bytes: the widest K that fits, never fewer than the min(M, 16) slots
 * of nbd_step_workspace_bytes(n), below which it returns NBD_E_WORKSPACE. Every K gives the same terms in a fixed
 * order of its own: deterministic, equal to any other K to summation-order rounding. */
size_t nbd_step_workspace_pref_bytes(int n);

/* One whole LeapFrogSimulator.step (simulation.py:153-170) on one GPU:
 *   kick-drift-pack -> all-pairs force -> kick, three launches on `stream`.
 * acc_in is a(t) (read), acc_out receives a(t+dt) (may alias acc_in).
 * posm: scratch float4[nbd_posm_padded_len(n)]; workspace as nbd_step_workspace_bytes(n). */
int nbd_leapfrog_step_f32(float* pos, float* vel, const float* acc_in, float* acc_out,
                          const float* mass, int n, float dt_half, float dt, float softening_sq,
                          float g_const, float* posm, void* workspace, size_t workspace_bytes,
                          nbd_stream_t stream);

/* Same as nbd_leapfrog_step_f32, additionally recording two caller-created hipEvent_t handles on
 * `stream` immediately before and after the all-pairs force kernel (NULL = skip). Measurement
 * hook for bench.py's roofline leg; the arithmetic and launches are identical. */
int nbd_leapfrog_step_ev_f32(float* pos, float* vel, const float* acc_in, float* acc_out,
                             const float* mass, int n, float dt_half, float dt, float softening_sq,
                             float g_const, float* posm, void* workspace, size_t workspace_bytes,
                             nbd_stream_t stream, void* ev_force_begin, void* ev_force_end);
/* The same step for a system whose bodies all have the SAME mass (round 3; the published configurations: Plummer,
 * m = 1 / N): the mass factors out of the force sum, a = (G m) sum_j d_ij s_ij^3, so the force kernel drops its per-pair
 * multiply by m_j (11 packed fp32 ops + 2 v_rsq_f32 per source and pair of targets instead of 12 + 2) and g_const *
 * mass_value is applied once, to the finished sum. The differences r_j - r_i stay the exact fp32 subtractions of
 * simulation.py:80; one multiplication per sum rounds differently from one per term. The caller vouches that every
 * entry of `mass` equals mass_value. From n = 65 536 on (softening_sq >= 1e-24) the force evaluates each off-diagonal pair
 * once and feeds both rows (Newton's third law; nbd_accel_sym_uniform_f32), same terms summed in another fixed order.
 * Workspace: nbd_step_workspace_bytes(n) at least, nbd_step_workspace_pref_bytes(n) for the one-launch plan. */
int nbd_leapfrog_step_uniform_f32(float* pos, float* vel, const float* acc_in, float* acc_out, const float* mass,
                                  float mass_value, int n, float dt_half, float dt, float softening_sq, float g_const,
                                  float* posm, void* workspace, size_t workspace_bytes, nbd_stream_t stream,
                                  void* ev_force_begin, void* ev_force_end);

/* The force of nbd_leapfrog_step_uniform_f32's symmetric path on its own (tests, profiling): acc = g_const * mass_value *
 * sum_j d_ij s_ij^3 over all n bodies of posm, each off-diagonal pair evaluated once (Newton's third law). Needs
 * n >= 2048 and softening_sq >= 1e-24 (else NBD_E_UNSUPPORTED). Deterministic. variant: the register shape (0: 4 source
 * groups per tile pair; 1: 2 source groups; 2: the step's, two sources per step packed by source), same sums in another
 * order. Workspace: nbd_accel_sym_workspace_bytes(n) at least (min(M, 16) slots of n rows, one more when n is no multiple
 * of 2048); a larger one widens the plan slot by slot as nbd_step_workspace_pref_bytes describes. */
size_t nbd_accel_sym_workspace_bytes(int n);
int nbd_accel_sym_uniform_f32(const float* posm, int n, float softening_sq, float g_const, float mass_value,
                              float* acc_out, void* workspace, size_t workspace_bytes, int variant, nbd_stream_t stream);
/* The same force as the step launches it: variant 2, and where the workspace gives every round a slot of its own (K = M)
 * the diagonal blocks run as the trailing workgroups of the one pair launch instead of in a launch in front of it. Same
 * arguments, checks and workspace; bit-identical to variant 2 on the same workspace size. */
int nbd_accel_sym_tail_uniform_f32(const float* posm, int n, float softening_sq, float g_const, float mass_value,
                                   float* acc_out, void* workspace, size_t workspace_bytes, nbd_stream_t stream);

/* One whole EulerSimulator.step (simulation.py:173-187): force -> kick(dt) -> drift(dt). */
int nbd_euler_step_f32(float* pos, float* vel, float* acc_out, const float* mass, int n, float dt,
                       float softening_sq, float g_const, float* posm, void* workspace,
                       size_t workspace_bytes, nbd_stream_t stream);

/* Bytes of scratch nbd_energy_f32 needs. */
size_t nbd_energy_workspace_bytes(int n);

/* BaseSimulator.compute_energies (simulation.py:91-115):
 *   K = sum_i 0.5 m_i |v_i|^2 ;  U = sum_{i<j} -G m_i m_j / (|r_i - r_j| + softening).
 * out_uk: device double[2] = {U, K} (pair sums are accumulated in fp64 from fp32 terms). */
int nbd_energy_f32(const float* posm, const float* vel, int n, float softening, float g_const,
                   double* out_uk, void* workspace, size_t workspace_bytes, nbd_stream_t stream);

/* ---------------------------------------------- consistent-potential diagnostics (csrc/direct_diag.hip)
 * An extension (the reference has nbd_energy_f32's convention only). The force above is the gradient of the Plummer
 * potential, not of -G m_i m_j / (|r| + softening): the energy an exact integrator conserves is K + 1/2 sum m_i phi_i with
 *   phi[i] = -g_const * sum_{j != i} m_j (|r_j - r_i|^2 + softening_sq)^(-1/2),
 * the pair with global index j == tgt_global_offset + i excluded by index. Arguments as nbd_accel_f32 (rectangular:
 * sources, targets, the targets' offset in the source numbering); phi_out: double[n_tgt]. The pair term is fp32 (exact
 * differences, fma, v_rsq_f32); no fp32 sum runs past one 64-source chunk, everything above it and the factor -g_const
 * are fp64, in a fixed order: bit-identical run to run. Coincident distinct bodies with softening_sq = 0 give -inf.
 * Workspace: nbd_potential_workspace_bytes(n_src, n_tgt), 8-byte aligned. n_src = 0 gives zeros. */
size_t nbd_potential_workspace_bytes(int n_src, int n_tgt);
int nbd_potential_f32(const float* posm_src, int n_src, const float* posm_tgt, int n_tgt, int tgt_global_offset,
                      float softening_sq, float g_const, double* phi_out, void* workspace, size_t workspace_bytes,
                      nbd_stream_t stream);
/* The conserved quantities of the n bodies of posm (packed {x,y,z,m}), vel (n,3) and phi (double[n], as above):
 * out_row = device double[16] = {M, Cx, Cy, Cz, Px, Py, Pz, Lx, Ly, Lz, K, U, E, Q, 0, 0} with M = sum m,
 * C = sum m x / M, P = sum m v, L = sum m x cross v, K = sum 1/2 m |v|^2, U = 1/2 sum m phi, E = K + U, Q = -2 K / U
 * (C = 0 when M = 0, Q = 0 when U = 0). Every product is formed in fp64 from the fp32 state and summed in a fixed order;
 * K therefore differs from nbd_energy_f32's (fp32 products) in the last digits. n = 0 gives a row of zeros. */
int nbd_invariants_f64(const float* posm, const float* vel, const double* phi, int n, double* out_row,
                       nbd_stream_t stream);

/* ---------------------------------------------------------------- batched direct integrator
 * An ensemble of S >= 1 independent systems ("scenes") in one set of arrays: scene s owns bodies
 * [offsets[s], offsets[s + 1]) of pos / vel / acc (n,3) and mass (n,); offsets is a HOST int array of S + 1 entries,
 * offsets[0] = 0, non-decreasing (zero-body scenes allowed). Each body feels only the bodies of its own scene, with
 * that scene's G, softening and dt: the per-scene parameters are DEVICE fp32 arrays of S entries. The packed sources
 * of a scene start at a multiple of NBD_SRC_PAD rows of `posm` (float4[posm_rows], 16-byte aligned). Each entry
 * validates offsets on the host (negative / decreasing / S <= 0: NBD_E_BADARG) before it touches the device.
 * A scene's work and summation order depend on its own size only: its results are bit-identical alone or with any
 * other scenes, at any position, run to run (no float atomics). No host syncs, no memsets: capturable.
 *
 * Host-only plan query: work items (one per scene x 128-target group x slab), packed rows, and the bytes of the
 * device plan and of the workspace. */
int nbd_batch_plan(const int* offsets, int n_scenes, int* n_items, int* posm_rows, size_t* plan_bytes,
                   size_t* workspace_bytes);
/* Host-only: writes the plan (plan_bytes as nbd_batch_plan reported) into HOST memory; the caller copies it to a
 * 16-byte-aligned device buffer once and passes that buffer, with the same offsets, to the entries below. */
int nbd_batch_plan_fill(const int* offsets, int n_scenes, void* plan, size_t plan_bytes);
/* posm = {x, y, z, m} of every scene (zeros in each scene's padding). */
int nbd_batch_pack_posm_f32(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const float* pos,
                            const float* mass, float* posm, nbd_stream_t stream);
/* BaseSimulator.compute_accelerations per scene (simulation.py:71-89): pack posm, then
 * acc_i = G_s sum_{j != i, j in s} m_j d_ij (|d_ij|^2 + eps_s^2)^(-3/2) (i == j dropped by index). */
int nbd_batch_accel_f32(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const float* pos,
                        const float* mass, const float* softening_sq, const float* g_const, float* acc_out,
                        float* posm, void* workspace, size_t workspace_bytes, nbd_stream_t stream);
/* LeapFrogSimulator.step per scene (simulation.py:153-170), three launches for all scenes: kick(dt_half_s) +
 * drift(dt_s) + pack, the segmented force, the slab sum with G_s and the second kick fused. Leaves posm = the new
 * positions. acc_in may alias acc_out. */
int nbd_batch_leapfrog_step_f32(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, float* pos,
                                float* vel, const float* acc_in, float* acc_out, const float* mass, const float* dt_half,
                                const float* dt, const float* softening_sq, const float* g_const, float* posm,
                                void* workspace, size_t workspace_bytes, nbd_stream_t stream);
/* EulerSimulator.step per scene (simulation.py:173-187): force -> kick(dt_s) -> drift(dt_s); leaves posm = the
 * moved positions. */
int nbd_batch_euler_step_f32(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, float* pos,
                             float* vel, float* acc_out, const float* mass, const float* dt, const float* softening_sq,
                             const float* g_const, float* posm, void* workspace, size_t workspace_bytes,
                             nbd_stream_t stream);
/* compute_energies per scene (simulation.py:91-115) from posm (as packed by the entries above) and vel: out_uk is a
 * device double[S][2] = {U_s, K_s}; a zero-body scene gives {0, 0}. */
int nbd_batch_energies(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const float* posm,
                       const float* vel, const float* softening, const float* g_const, double* out_uk, void* workspace,
                       size_t workspace_bytes, nbd_stream_t stream);
/* nbd_potential_f32 per scene (csrc/direct_diag.hip) from posm as packed by the entries above: phi_out is a device
 * double[N_total] in body order, scene s with its softening_sq[s] and g_const[s]. A scene's values are bit-identical to
 * nbd_potential_f32 on that scene alone. Workspace: the one nbd_batch_plan reports is large enough (8-byte aligned). */
int nbd_batch_potential_f32(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const float* posm,
                            const float* softening_sq, const float* g_const, double* phi_out, void* workspace,
                            size_t workspace_bytes, nbd_stream_t stream);
/* nbd_invariants_f64 per scene: out_rows is a device double[S][16]; a zero-body scene gives a row of zeros. A scene's
 * row is bit-identical to nbd_invariants_f64 on that scene alone. */
int nbd_batch_invariants_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const float* posm,
                             const float* vel, const double* phi, double* out_rows, nbd_stream_t stream);

/* Hermite per scene (csrc/direct_batch_hermite.hip): the scheme of nbd_hermite_step_f32 below applied to every scene,
 * three launches for all scenes, on the plan above. A scene's pos / vel / acc / jerk are bit-identical to
 * nbd_hermite_step_f32 (nbd_accel_jerk_f32 after nbd_hermite_pack_f32) on that scene alone with the same parameters.
 * Host-only: the bytes of the Hermite workspace (16-byte aligned: packed velocities float4[posm_rows], then the
 * acceleration + jerk partial sums); NBD_E_UNSUPPORTED when those sums outgrow the kernels' int offsets. */
int nbd_batch_hermite_workspace_bytes(const int* offsets, int n_scenes, size_t* bytes);
/* acc_out, jerk_out (N, 3) of the current state of every scene: a plain pack of (x, v) into posm and the workspace, the
 * acceleration + jerk, the fixed-order slab sum with G_s. Leaves posm = {x, m}. */
int nbd_batch_accel_jerk_f32(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const float* pos,
                             const float* vel, const float* mass, const float* softening_sq, const float* g_const,
                             float* acc_out, float* jerk_out, float* posm, void* workspace, size_t workspace_bytes,
                             nbd_stream_t stream);
/* One Hermite step of every scene: predict + pack, acceleration + jerk at the predicted state, slab sum + corrector.
 * hdt: device fp32 [5][S] table of each scene's (dt, dt/2, dt^2/2, dt^3/6, dt^2/12), each formed from the double dt
 * and rounded once. Writes pos, vel (in place), acc_out, jerk_out and posm = {x1, m}. acc_in may alias acc_out and
 * jerk_in may alias jerk_out. */
int nbd_batch_hermite_step_f32(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, float* pos,
                               float* vel, const float* acc_in, const float* jerk_in, float* acc_out, float* jerk_out,
                               const float* mass, const float* hdt, const float* softening_sq, const float* g_const,
                               float* posm, void* workspace, size_t workspace_bytes, nbd_stream_t stream);

/* ---- double-precision Hermite per scene (csrc/direct_batch_hermite_f64.hip): "double-precision Hermite" below applied
 * to every scene of a batch, one set of launches for all scenes. State, masses, a, j: double; offsets as above. A scene's
 * pos / vel / acc / jerk, energies, potentials and invariants are bit-identical to the nbd_*_f64 entries of
 * "double-precision Hermite" on that scene alone with the same parameters, wherever it stands in the batch.
 *   plan   : a work list of its own (NOT the one of nbd_batch_plan): one item per scene x group of 64 targets x slab, the
 *            slab count of a scene being nbd_hermite_f64_plan's for its size; same layout, same rules (16-byte aligned
 *            device buffer, plan_bytes as reported). NBD_E_UNSUPPORTED when the items, the rows or the doubles of the
 *            partial sums outgrow the kernels' int offsets.
 *   posd, veld : double[rows][4], 32-byte aligned: {x, y, z, m} and {vx, vy, vz, 0}, every scene padded to whole chunks of
 *            NBD_SRC_PAD rows with zero rows (rows as nbd_batch_f64_plan reports).
 *   params : DEVICE double[NBD_BATCH_F64_PARAM_ROWS][S], 8-byte aligned, row r of scene s at params[r * S + s]; rows:
 *            G, softening^2, softening, dt, dt/2, dt^2/2, dt^3/6, dt^2/12 -- the doubles nbd_hermite_step_f64 forms from
 *            its dt (0.5*dt, 0.5*dt*dt, dt*dt*dt/6.0, dt*dt/12.0). Every per-scene scalar is read from this table by the
 *            kernels: a step can be captured into a graph, and a changed parameter is a rewrite of the table.
 *   workspace : nbd_batch_f64_workspace_bytes, 8-byte aligned (6 doubles per body and slab); it may hold anything.
 * Argument errors return NBD_E_BADARG (NBD_E_WORKSPACE for the workspace) before any launch. No atomics, no memsets, no
 * host syncs. */
#define NBD_BATCH_F64_PARAM_ROWS 8
/* Host-only: work items, packed rows and the bytes of the device plan. */
int nbd_batch_f64_plan(const int* offsets, int n_scenes, int* n_items, int* rows, size_t* plan_bytes);
/* Host-only: the bytes of the workspace of every entry below. */
int nbd_batch_f64_workspace_bytes(const int* offsets, int n_scenes, size_t* bytes);
/* Host-only: writes the plan into HOST memory (as nbd_batch_plan_fill). */
int nbd_batch_f64_plan_fill(const int* offsets, int n_scenes, void* plan, size_t plan_bytes);
/* posd = {x, m}, veld = {v, 0} of every scene (zero rows in each scene's padding): one launch. */
int nbd_batch_pack_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const double* pos,
                       const double* vel, const double* mass, double* posd, double* veld, nbd_stream_t stream);
/* acc_out, jerk_out (N, 3) of the current state of every scene: the pack above, the acceleration + jerk, the slab sum in
 * slab order with G_s. Leaves posd = {x, m}, veld = {v, 0}. */
int nbd_batch_accel_jerk_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const double* pos,
                             const double* vel, const double* mass, const double* params, double* acc_out,
                             double* jerk_out, double* posd, double* veld, void* workspace, size_t workspace_bytes,
                             nbd_stream_t stream);
/* One Hermite step of every scene, three launches: pos, vel in place; acc_out, jerk_out = a1, j1 at the predicted state
 * (acc_in may alias acc_out, jerk_in may alias jerk_out); posd = {x1, m}; veld is scratch. */
int nbd_batch_hermite_step_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, double* pos,
                               double* vel, const double* acc_in, const double* jerk_in, double* acc_out,
                               double* jerk_out, const double* mass, const double* params, double* posd, double* veld,
                               void* workspace, size_t workspace_bytes, nbd_stream_t stream);
/* nbd_energy_f64 per scene from posd (as the entries above leave it) and vel: out_uk is a device double[S][2] =
 * {U_s, K_s}; a zero-body scene gives {0, 0}. */
int nbd_batch_energies_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const double* posd,
                           const double* vel, const double* params, double* out_uk, void* workspace,
                           size_t workspace_bytes, nbd_stream_t stream);
/* nbd_potential_f64 per scene: phi_out is a device double[N_total] in body order. */
int nbd_batch_potential_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const double* posd,
                            const double* params, double* phi_out, void* workspace, size_t workspace_bytes,
                            nbd_stream_t stream);
/* nbd_invariants_state_f64 per scene: out_rows is a device double[S][16]; a zero-body scene gives a row of zeros. */
int nbd_batch_invariants_state_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes,
                                   const double* pos, const double* vel, const double* mass, const double* phi,
                                   double* out_rows, nbd_stream_t stream);

/* ---- 6th-order Hermite per scene (csrc/direct_batch_hermite_f64.hip): "6th-order Hermite" below applied to every scene
 * of a batch, one set of launches for all scenes. A scene's pos / vel / acc / jerk / snap / crackle are bit-identical to
 * the nbd_*hermite6* / nbd_accel_jerk_snap_f64 entries on that scene alone with the same parameters, wherever it stands
 * in the batch.
 *   plan   : the layout, the items, the rows and the plan_bytes of nbd_batch_f64_plan (ask it for them), filled by
 *            nbd_batch_hermite6_f64_plan_fill: only each scene's first workspace double differs, counting
 *            double[slabs][9][n_s] per scene. The float64 diagnostic entries above (nbd_batch_energies_f64,
 *            nbd_batch_potential_f64, nbd_batch_invariants_state_f64, nbd_batch_pack_f64, nbd_batch_accel_jerk_f64) run
 *            unchanged on this plan with this workspace and this table: they read a scene's workspace offset from the
 *            plan, use the front of its region, and read rows 0..2 of the table.
 *   posd, veld, accd : double[rows][4], 32-byte aligned: {x, y, z, m}, {vx, vy, vz, 0} and {ax, ay, az, 0}, padded as above.
 *   params : DEVICE double[NBD_BATCH_H6_PARAM_ROWS][S], 8-byte aligned, row r of scene s at params[r * S + s]; rows:
 *            G, softening^2, softening (as NBD_BATCH_F64_PARAM_ROWS' first three), then the doubles nbd_hermite6_step_f64
 *            forms from its dt, with dt2 = dt*dt and dt3 = dt2*dt: dt, 0.5*dt, 0.5*dt2, dt3/6.0, dt2*dt2/24.0,
 *            dt2*dt3/120.0, dt2/10.0, dt3/120.0, dt2, dt3. No kernel takes a per-scene scalar by value.
 *   workspace : nbd_batch_hermite6_f64_workspace_bytes, 8-byte aligned (9 doubles per body and slab); it may hold anything.
 * Argument errors return NBD_E_BADARG (NBD_E_WORKSPACE for the workspace) before any launch. No atomics, no memsets, no
 * host syncs. */
#define NBD_BATCH_H6_PARAM_ROWS 13
/* Host-only: writes the 9-row plan into HOST memory; plan_bytes as nbd_batch_f64_plan reports. */
int nbd_batch_hermite6_f64_plan_fill(const int* offsets, int n_scenes, void* plan, size_t plan_bytes);
/* Host-only: the bytes of the workspace of the entries below (1.5 x nbd_batch_f64_workspace_bytes). */
int nbd_batch_hermite6_f64_workspace_bytes(const int* offsets, int n_scenes, size_t* bytes);
/* posd = {x, m}, veld = {v, 0}, accd = {a, 0} of every scene (acc == NULL: accd = 0; zero rows in each scene's padding):
 * one launch. */
int nbd_batch_hermite6_pack_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const double* pos,
                                const double* vel, const double* acc, const double* mass, double* posd, double* veld,
                                double* accd, nbd_stream_t stream);
/* acc_out, jerk_out, snap_out (N, 3) of every scene from the packed rows (nbd_accel_jerk_snap_f64 per scene at the plan's
 * slab count): the evaluation and the slab sum in slab order with G_s, two launches. */
int nbd_batch_accel_jerk_snap_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes,
                                  const double* posd, const double* veld, const double* accd, const double* params,
                                  double* acc_out, double* jerk_out, double* snap_out, void* workspace,
                                  size_t workspace_bytes, nbd_stream_t stream);
/* One 6th-order Hermite step of every scene, three launches (nbd_hermite6_step_f64 per scene): pos, vel in place; every
 * output may alias its input; posd = {x1, m}; veld and accd are scratch. */
int nbd_batch_hermite6_step_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, double* pos,
                                double* vel, const double* acc_in, const double* jerk_in, const double* snap_in,
                                const double* crackle_in, double* acc_out, double* jerk_out, double* snap_out,
                                double* crackle_out, const double* mass, const double* params, double* posd,
                                double* veld, double* accd, void* workspace, size_t workspace_bytes,
                                nbd_stream_t stream);

/* ------------------------------------------------------------ 4th-order Hermite integrator (csrc/direct_hermite.hip)
 * An extension (the reference has Euler and leapfrog only): the shared-timestep predictor-corrector of Makino & Aarseth
 * (1992), one acceleration + jerk evaluation per step, fp32 state. With r_ij = x_j - x_i, v_ij = v_j - v_i and
 * s = (|r_ij|^2 + softening_sq)^(-1/2):  a_i = G sum_{j!=i} m_j r_ij s^3,
 * j_i = G sum_{j!=i} m_j (v_ij s^3 - 3 (r_ij.v_ij) s^5 r_ij). Below softening_sq = 1e-24 the i == j term is dropped by
 * index, as in nbd_accel_f32. The fp32 step constants (dt, dt/2, dt^2/2, dt^3/6, dt^2/12) are formed from the double dt
 * and rounded once. Deterministic (fixed-order slab sums, no atomics) and capturable (no memsets, no host syncs).
 * Workspace: nbd_hermite_workspace_bytes(n), 16-byte aligned. */
size_t nbd_hermite_workspace_bytes(int n);
/* posm = {x_p, m}, velp = {v_p, 0}: float4[nbd_posm_padded_len(n)] each, zero padding. With acc and jerk the predicted
 * state x_p = x + v dt + a dt^2/2 + j dt^3/6, v_p = v + a dt + j dt^2/2; with both null a plain pack of (x, v). */
int nbd_hermite_pack_f32(const float* pos, const float* vel, const float* acc, const float* jerk, const float* mass,
                         int n, double dt, float* posm, float* velp, nbd_stream_t stream);
/* The force alone (tests, profiling): acc_out and jerk_out (n,3) of all n bodies of posm / velp. variant: the register
 * shape of the kernel (0: the step's, two sources in flight; 1: four), same sums. */
int nbd_accel_jerk_f32(const float* posm, const float* velp, int n, float softening_sq, float g_const, float* acc_out,
                       float* jerk_out, void* workspace, size_t workspace_bytes, int variant, nbd_stream_t stream);
/* One step: predict + pack, acceleration + jerk at the predicted state, slab sum + corrector (three launches). Writes
 * pos, vel (in place), acc_out, jerk_out (= a1, j1 at the predicted state, carried into the next step) and
 * posm = {x1, m}. acc_in may alias acc_out and jerk_in may alias jerk_out. posm: float4[nbd_posm_padded_len(n)]. */
int nbd_hermite_step_f32(float* pos, float* vel, const float* acc_in, const float* jerk_in, float* acc_out,
                         float* jerk_out, const float* mass, int n, double dt, float softening_sq, float g_const,
                         float* posm, void* workspace, size_t workspace_bytes, nbd_stream_t stream);

/* ---- range-sharded Hermite step (csrc/direct_hermite_shard.hip): one rank of a range partition owns bodies
 * [lo, lo + n_local) of n_total and advances them by the scheme above. The exchanged row is 8 floats,
 * {x_p, y_p, z_p, m, vx_p, vy_p, vz_p, 0}: the predicted state and the mass, ONE all-gather per step.
 *   send : float[send_rows][8], the rank's own rows, zero behind n_local; send_rows >= nbd_posm_padded_len(n_local)
 *          (a ragged partition sends more rows than it owns: they are the zeros)
 *   all  : float[nbd_posm_padded_len(n_total)][8], every rank's rows in global order, zero behind n_total
 * A step is, in the caller's stream:
 *   nbd_hermite_shard_predict_f32       hermite predictor of the own bodies -> send
 *   (start the all-gather of send into all)
 *   nbd_hermite_shard_force_local_f32   own bodies as sources (reads send only); runs while the gather is in flight
 *   (wait for the gather)
 *   nbd_hermite_shard_force_remote_f32  all other bodies as sources (rows [lo, lo + n_local) of `all` are never used:
 *                                       whole 64-row chunks inside the range are not read, the rest of it is dropped by
 *                                       select), then a launch of its own: a1, j1 = G * (fixed-order sum of every slab,
 *                                       local ones first) and the corrector of the own rows
 * Four launches. Any lo and n_local; n_local == 0 is a no-op returning 0; a rank that owns everything (a one-rank group)
 * has no remote launch. Below softening_sq = 1e-24 the i == j term is dropped by index. The workspace holds the partial
 * sums (6 floats per target and slab) between the two force calls of a step: nbd_hermite_shard_workspace_bytes, the same
 * buffer for both. A wave's sequential fp32 chain stays <= 4096 sources. Deterministic and capturable. */
int nbd_hermite_shard_plan(int n_total, int lo, int n_local, int* slabs_local, int* chunks_per_wave_local,
                           int* slabs_remote, int* chunks_per_wave_remote);
size_t nbd_hermite_shard_workspace_bytes(int n_total, int lo, int n_local);
/* send rows [0, n_local) = the state predicted over dt from (acc, jerk) with the masses (mass: the rank's n_local), rows
 * [n_local, send_rows) = 0. With acc and jerk both null a plain pack of (pos, vel), as nbd_hermite_pack_f32. */
int nbd_hermite_shard_predict_f32(const float* pos, const float* vel, const float* acc, const float* jerk,
                                  const float* mass, int n_local, double dt, float* send, int send_rows,
                                  nbd_stream_t stream);
int nbd_hermite_shard_force_local_f32(const float* send, int n_local, float softening_sq, void* workspace,
                                      size_t workspace_bytes, int n_total, int lo, nbd_stream_t stream);
/* pos non-null: the corrector -- pos, vel (n_local,3) in place from acc_in, jerk_in, dt; acc_out, jerk_out = a1, j1 at
 * the predicted state (acc_in may alias acc_out, jerk_in may alias jerk_out). pos null: the force on its own, acc_out
 * and jerk_out only (vel, acc_in, jerk_in and dt are not used). */
int nbd_hermite_shard_force_remote_f32(const float* all, int n_total, const float* send, int n_local, int lo,
                                       float softening_sq, float g_const, float* pos, float* vel, const float* acc_in,
                                       const float* jerk_in, float* acc_out, float* jerk_out, double dt, void* workspace,
                                       size_t workspace_bytes, nbd_stream_t stream);

/* ---- double-precision Hermite (csrc/direct_hermite_f64.hip): the step of nbd_hermite_step_f32 and the diagnostics of a
 * system with fp64 state, fp64 scalars and fp64 pair arithmetic throughout (the reciprocal square root is v_rsq_f64
 * refined in fp64 to about 1 ulp; the step constants are the doubles formed from dt). An extension, used only when asked
 * for; the fp32 entries are untouched by it. The packed sources are rows of 4 doubles, 32-byte aligned:
 *   posd : double[nbd_posm_padded_len(n)][4] = {x, y, z, m}, veld : the same shape = {vx, vy, vz, 0}, zero rows behind n.
 * i == j is dropped by index below softening_sq = 1e-24 and in the chunk that holds the targets' own rows, elsewhere by
 * the term being an exact zero; a massless body is a valid source and target. Deterministic (fixed-order sums, no
 * atomics; the workspace may hold anything on entry) and capturable (no memsets, no host syncs).
 * Workspace of every entry: nbd_hermite_f64_workspace_bytes(n), 8-byte aligned (6 doubles per body and slab). */
size_t nbd_hermite_f64_workspace_bytes(int n);
/* The launch geometry at n bodies: groups of 64 targets, source slabs, the largest chunk count of a wave. */
int nbd_hermite_f64_plan(int n, int* groups, int* slabs, int* chunks_per_wave);
/* posd = {x_p, m}, veld = {v_p, 0}: the state predicted over dt from (acc, jerk), or a plain pack of (pos, vel) when both
 * are null. pos, vel, acc, jerk: double (n,3); mass: double (n). */
int nbd_hermite_f64_pack(const double* pos, const double* vel, const double* acc, const double* jerk, const double* mass,
                         int n, double dt, double* posd, double* veld, nbd_stream_t stream);
/* The force alone: acc_out and jerk_out, double (n,3), of all n bodies of posd / veld. slabs: 0 for the plan's split of
 * the sources, or an explicit slab count in [1, 64] (tests: it sets how many chunks a wave walks; the workspace then
 * needs slabs * 6 * n doubles). */
int nbd_accel_jerk_f64(const double* posd, const double* veld, int n, double softening_sq, double g_const,
                       double* acc_out, double* jerk_out, void* workspace, size_t workspace_bytes, int slabs,
                       nbd_stream_t stream);
/* One step, three launches, as nbd_hermite_step_f32: pos, vel in place; acc_out, jerk_out = a1, j1 at the predicted state
 * (acc_in may alias acc_out, jerk_in may alias jerk_out); posd = {x1, m}; veld is scratch. */
int nbd_hermite_step_f64(double* pos, double* vel, const double* acc_in, const double* jerk_in, double* acc_out,
                         double* jerk_out, const double* mass, int n, double dt, double softening_sq, double g_const,
                         double* posd, double* veld, void* workspace, size_t workspace_bytes, nbd_stream_t stream);
/* out_uk = {U, K} in nbd_energy_f32's (the reference's) convention, U = sum_{i<j} -G m_i m_j / (|r_ij| + softening),
 * K = sum 1/2 m |v|^2, from posd and vel double (n,3). n = 0 gives {0, 0}. */
int nbd_energy_f64(const double* posd, const double* vel, int n, double softening, double g_const, double* out_uk,
                   void* workspace, size_t workspace_bytes, nbd_stream_t stream);
/* phi_out[i] = -G sum_{j != i} m_j (|r_ij|^2 + softening_sq)^(-1/2), double (n): nbd_potential_f32's potential. */
int nbd_potential_f64(const double* posd, int n, double softening_sq, double g_const, double* phi_out, void* workspace,
                      size_t workspace_bytes, nbd_stream_t stream);
/* nbd_invariants_f64's row {M, C (3), P (3), L (3), K, U, E, Q, 0, 0} from an fp64 state (pos, vel double (n,3), mass
 * double (n)) and its potentials phi (nbd_potential_f64): the same sums in the same order. */
int nbd_invariants_state_f64(const double* pos, const double* vel, const double* mass, const double* phi, int n,
                             double* out_row, nbd_stream_t stream);

/* ---- 6th-order Hermite (csrc/direct_hermite_f64.hip): the shared-timestep 6th-order Hermite step (Nitadori & Makino
 * 2008) in the number format of "double-precision Hermite" above -- fp64 state, scalars, pair arithmetic and sums; there
 * is no fp32 form. The force evaluation carries the snap s = d^2 a / dt^2 and streams a third array of packed rows,
 *   accd : double[nbd_posm_padded_len(n)][4] = {ax, ay, az, 0}, 32-byte aligned, zero rows behind n, as veld.
 * With r = x_j - x_i, v = v_j - v_i, a = a_j - a_i, s = (|r|^2 + softening_sq)^(-1/2), w = m_j s^3, alpha = (r.v) s^2 and
 * gamma = (v.v + r.a) s^2 the pair terms are A = w r, J = w v - 3 alpha w r, S = w a - 6 alpha w v + (15 alpha^2 -
 * 3 gamma) w r. i == j, massless bodies, determinism and capturability as above. The acceleration and the jerk are the
 * bits of nbd_accel_jerk_f64 at the same slab count. */
/* plan_f64(n).slabs * 9 * n * 8: 9 doubles per body and slab (the slab count is nbd_hermite_f64_plan's). */
size_t nbd_hermite6_f64_workspace_bytes(int n);
/* posd = {x_p, m}, veld = {v_p, 0}, accd = {a_p, 0}: the state predicted over dt by the Taylor series to the crackle
 * c = d^3 a / dt^3. With jerk, snap and crackle all null a plain pack of (pos, vel, acc), and a null acc gives zero rows;
 * jerk, snap and crackle are given together, with acc. All arrays double (n,3); mass: double (n). */
int nbd_hermite6_f64_pack(const double* pos, const double* vel, const double* acc, const double* jerk,
                          const double* snap, const double* crackle, const double* mass, int n, double dt, double* posd,
                          double* veld, double* accd, nbd_stream_t stream);
/* The force alone: acc_out, jerk_out and snap_out, double (n,3), of all n bodies of posd / veld / accd. slabs: 0 for the
 * plan's split of the sources, or an explicit slab count in [1, 64] (the workspace then needs slabs * 9 * n doubles). */
int nbd_accel_jerk_snap_f64(const double* posd, const double* veld, const double* accd, int n, double softening_sq,
                            double g_const, double* acc_out, double* jerk_out, double* snap_out, void* workspace,
                            size_t workspace_bytes, int slabs, nbd_stream_t stream);
/* One step, three launches (predict, evaluate, correct): pos, vel in place; acc_out, jerk_out, snap_out = a1, j1, s1 at
 * the predicted state; crackle_out = the third derivative at t1 of the quintic through (a, j, s) at both ends. Every
 * output may alias its input. posd = {x1, m}; veld and accd are scratch. Workspace: nbd_hermite6_f64_workspace_bytes(n),
 * 8-byte aligned. */
int nbd_hermite6_step_f64(double* pos, double* vel, const double* acc_in, const double* jerk_in, const double* snap_in,
                          const double* crackle_in, double* acc_out, double* jerk_out, double* snap_out,
                          double* crackle_out, const double* mass, int n, double dt, double softening_sq, double g_const,
                          double* posd, double* veld, double* accd, void* workspace, size_t workspace_bytes,
                          nbd_stream_t stream);

/* ---- double-precision leapfrog (csrc/direct_leapfrog_f64.hip): the steps of nbd_leapfrog_step_f32 and
 * nbd_euler_step_f32 and the acceleration on its own, in the number format of "double-precision Hermite" above: fp64
 * state, scalars, pair arithmetic and sums, posd as described there (no veld: no velocity row is read by the force).
 * Every product and sum of the O(N) updates rounds on its own. Deterministic (the workspace may hold anything on entry)
 * and capturable. A workspace of nbd_hermite_f64_workspace_bytes(n) bytes is large enough for every entry at slabs = 0. */
/* slabs * 3 * n doubles; slabs = 0: the slab count of nbd_hermite_f64_plan(n). 0 for n <= 0 or slabs outside [0, 64]. */
size_t nbd_accel_f64_workspace_bytes(int n, int slabs);
/* acc_out, double (n,3), of all n bodies of posd: for every n and every slab count (0: the plan's; [1, 64]: explicit, as
 * nbd_accel_jerk_f64 takes one) the bits of nbd_accel_jerk_f64's acc_out at that slab count. */
int nbd_accel_f64(const double* posd, int n, double softening_sq, double g_const, double* acc_out, void* workspace,
                  size_t workspace_bytes, int slabs, nbd_stream_t stream);
/* One kick-drift-kick step, three launches: v += dt_half acc_in, x += dt v, posd = {x, m}; acc_out = a(x); v += dt_half
 * acc_out. pos, vel in place; acc_in may alias acc_out; posd is left at the post-step positions. */
int nbd_leapfrog_step_f64(double* pos, double* vel, const double* acc_in, double* acc_out, const double* mass, int n,
                          double dt_half, double dt, double softening_sq, double g_const, double* posd, void* workspace,
                          size_t workspace_bytes, nbd_stream_t stream);
/* One Euler step, three launches, in the reference's order: posd = {x, m}; acc_out = a(x); v += dt acc_out, x += dt v.
 * posd is left at the positions from BEFORE the drift, as nbd_euler_step_f32 leaves posm. */
int nbd_euler_step_f64(double* pos, double* vel, double* acc_out, const double* mass, int n, double dt,
                       double softening_sq, double g_const, double* posd, void* workspace, size_t workspace_bytes,
                       nbd_stream_t stream);

/* ---- double-precision range-sharded Hermite step (csrc/direct_hermite_shard_f64.hip): "range-sharded Hermite step" in
 * the number format of "double-precision Hermite". State, masses, a, j, G, softening_sq, dt and the pair arithmetic are
 * fp64; a rank that owns every body gets nbd_accel_jerk_f64's bits. The exchanged row is 8 doubles (64 bytes),
 * {x_p, y_p, z_p, m, vx_p, vy_p, vz_p, 0}: ONE all-gather per step, read by the force kernels as it lands.
 *   send : double[send_rows][8], 32-byte aligned, the rank's own rows, zero behind n_local;
 *          send_rows >= nbd_posm_padded_len(n_local)
 *   all  : double[nbd_posm_padded_len(n_total)][8], 32-byte aligned, every rank's rows in global order, zero behind n_total
 * A step is the four launches of the fp32 entries, argument for argument: predict, (start the gather), force_local,
 * (wait for it), force_remote = the remote block (rows [lo, lo + n_local) of `all` are never used: whole 64-row chunks
 * inside the range are not read, the rest of it is dropped by select) + one launch that adds every slab in slab order,
 * local ones first, times G, and corrects the own rows. Any lo and n_local; n_local == 0 is a no-op returning 0; a rank
 * that owns everything has no remote launch. Below softening_sq = 1e-24 the i == j term is dropped by index.
 * slabs, slabs_local, slabs_remote: 0 for the plan's split of the source chunks (the local block: nbd_hermite_f64_plan
 * at n_local; the remote block: the same target groups, slabs for ~1024 workgroups while every wave keeps a chunk), or
 * an explicit slab count in [1, 64] as nbd_accel_jerk_f64 takes one (tests: it sets how many chunks a wave walks). Both
 * force calls of a step must be given the same slabs_local. The workspace holds the partial sums between them:
 * (slabs_local + slabs_remote) * 6 * n_local doubles, 8-byte aligned, nbd_hermite_shard_f64_workspace_bytes with the same
 * slab arguments (0 where an argument is out of range); force_local needs its slabs_local * 6 * n_local doubles of it.
 * It may hold anything on entry. Deterministic; no atomics, no memsets, no host syncs. */
int nbd_hermite_shard_f64_plan(int n_total, int lo, int n_local, int* slabs_local, int* chunks_per_wave_local,
                               int* slabs_remote, int* chunks_per_wave_remote);
size_t nbd_hermite_shard_f64_workspace_bytes(int n_total, int lo, int n_local, int slabs_local, int slabs_remote);
/* send rows [0, n_local) = the state predicted over dt from (acc, jerk) with the masses (mass: the rank's n_local), rows
 * [n_local, send_rows) = 0. With acc and jerk both null a plain pack of (pos, vel), as nbd_hermite_f64_pack. */
int nbd_hermite_shard_predict_f64(const double* pos, const double* vel, const double* acc, const double* jerk,
                                  const double* mass, int n_local, double dt, double* send, int send_rows,
                                  nbd_stream_t stream);
int nbd_hermite_shard_force_local_f64(const double* send, int n_local, double softening_sq, void* workspace,
                                      size_t workspace_bytes, int n_total, int lo, int slabs, nbd_stream_t stream);
/* pos non-null: the corrector -- pos, vel (n_local,3) in place from acc_in, jerk_in, dt; acc_out, jerk_out = a1, j1 at
 * the predicted state (acc_in may alias acc_out, jerk_in may alias jerk_out). pos null: the force on its own, acc_out
 * and jerk_out only (vel, acc_in, jerk_in and dt are not used). */
int nbd_hermite_shard_force_remote_f64(const double* all, int n_total, const double* send, int n_local, int lo,
                                       double softening_sq, double g_const, double* pos, double* vel,
                                       const double* acc_in, const double* jerk_in, double* acc_out, double* jerk_out,
                                       double dt, void* workspace, size_t workspace_bytes, int slabs_local,
                                       int slabs_remote, nbd_stream_t stream);

/* ---- 6th-order Hermite, range-sharded (csrc/direct_hermite_shard_f64.hip, with the 4th order): "6th-order Hermite" above for one rank of a
 * range partition, in the form of "double-precision range-sharded Hermite step": the five entries mirror the
 * nbd_hermite_shard_*_f64 entries in argument order and error codes, with the snap and the crackle beside the jerk. The
 * exchanged row is 12 doubles (96 bytes), {x_p, y_p, z_p, m, vx_p, vy_p, vz_p, 0, ax_p, ay_p, az_p, 0}: ONE all-gather
 * per step carries the three source arrays of nbd_accel_jerk_snap_f64, read by the force kernels as it lands.
 *   send : double[send_rows][12], 32-byte aligned, the rank's own rows, zero behind n_local;
 *          send_rows >= nbd_posm_padded_len(n_local)
 *   all  : double[nbd_posm_padded_len(n_total)][12], 32-byte aligned, every rank's rows in global order, zero behind
 *          n_total
 * The force kernels fetch whole 64-row chunks: both arrays must be allocated to those padded lengths. A step is predict,
 * (start the gather), force_local, (wait for it), force_remote = the remote block (rows [lo, lo + n_local) of `all` are
 * never used) + one launch that adds every slab in slab order, local ones first, times G, and corrects the own rows. Any
 * lo and n_local; n_local == 0 is a no-op returning 0; a rank that owns everything has no remote launch and gets
 * nbd_accel_jerk_snap_f64's bits; acc_out and jerk_out of any rank are nbd_hermite_shard_force_*_f64's bits at the same
 * slab counts. Slab arguments and the plan are those of the 4th-order entries; the workspace is (slabs_local +
 * slabs_remote) * 9 * n_local doubles, 8-byte aligned, and may hold anything on entry. Deterministic; no atomics, no
 * memsets, no host syncs. */
int nbd_hermite6_shard_f64_plan(int n_total, int lo, int n_local, int* slabs_local, int* chunks_per_wave_local,
                                int* slabs_remote, int* chunks_per_wave_remote);
size_t nbd_hermite6_shard_f64_workspace_bytes(int n_total, int lo, int n_local, int slabs_local, int slabs_remote);
/* send rows [0, n_local) = the state predicted over dt by the Taylor series to the crackle, with the masses (mass: the
 * rank's n_local), rows [n_local, send_rows) = 0. jerk, snap and crackle all null: a plain pack of (pos, vel, acc), and a
 * null acc gives a zero third quad pair; jerk, snap and crackle are given together, with acc (nbd_hermite6_f64_pack). */
int nbd_hermite6_shard_predict_f64(const double* pos, const double* vel, const double* acc, const double* jerk,
                                   const double* snap, const double* crackle, const double* mass, int n_local, double dt,
                                   double* send, int send_rows, nbd_stream_t stream);
int nbd_hermite6_shard_force_local_f64(const double* send, int n_local, double softening_sq, void* workspace,
                                       size_t workspace_bytes, int n_total, int lo, int slabs, nbd_stream_t stream);
/* pos non-null: the corrector -- pos, vel (n_local,3) in place from acc_in, jerk_in, snap_in, dt; acc_out, jerk_out,
 * snap_out = a1, j1, s1 at the predicted state, crackle_out = c1 (every output may alias its input). pos null: the force
 * on its own, acc_out, jerk_out and snap_out only (vel, the inputs, crackle_out and dt are not used). */
int nbd_hermite6_shard_force_remote_f64(const double* all, int n_total, const double* send, int n_local, int lo,
                                        double softening_sq, double g_const, double* pos, double* vel,
                                        const double* acc_in, const double* jerk_in, const double* snap_in,
                                        double* acc_out, double* jerk_out, double* snap_out, double* crackle_out,
                                        double dt, void* workspace, size_t workspace_bytes, int slabs_local,
                                        int slabs_remote, nbd_stream_t stream);

/* ------------------------------------------------ block-timestep Hermite integrator (csrc/direct_hermite_block.hip)
 * The scheme above with individual power-of-two steps (Makino & Aarseth 1992). One output interval dt is 2^K integer
 * ticks, K = max_level in [0, 20]. Body i keeps x, v, a, j at its last correction tick ticks[i] (int32) and a level
 * levels[i] in [0, K]; its step is d_i = 2^(K - k_i) ticks. sched is a device int[NBD_HBLOCK_SCHED_INTS] whose first
 * three entries are {t_next, n_act, clamped}: schedule writes t_next and n_act, the clamp counter is cumulative (zero it
 * once); the rest (current tick, level histogram) belongs to the entries. Every interval starts and ends with all
 * ticks at 0. A block step is schedule, then predict, force and correct (or nbd_hblock_step_f32, all three). Levels
 * come from the Aarseth criterion in fp64, quantised against the exact powers dt 2^-k; a level deeper than K (or a NaN
 * criterion) is clamped to K and counted. Workspace: nbd_hblock_workspace_bytes(n), 16-byte aligned; it holds the active
 * list and the partial sums between the calls of one block step. Eager-only (schedule reads back to the host). */
#define NBD_HBLOCK_SCHED_INTS 32
size_t nbd_hblock_workspace_bytes(int n);
/* ticks = 0 and levels from dt_i = (eta / 2) |a| / |j| for all n bodies; starts a new interval. */
int nbd_hblock_init_levels(const float* acc, const float* jerk, int n, double dt, double eta, int max_level, int* ticks,
                           int* levels, int* sched, nbd_stream_t stream);
/* t_next = min_i (ticks[i] + d_i) and the active list (in no fixed order) into the workspace. host_sched non-null:
 * sched[0..4) is copied there and the stream synchronised (the one readback of a block step; pinned memory is
 * fastest). */
int nbd_hblock_schedule(const int* levels, int n, int max_level, int* sched, void* workspace, size_t workspace_bytes,
                        int* host_sched, nbd_stream_t stream);
/* posm = {x_p, m}, velp = {v_p, 0} of every body predicted to t_next = sched[0] over (t_next - ticks[i]) dt / 2^K;
 * float4[nbd_posm_padded_len(n)] each, zero padding. */
int nbd_hblock_predict_f32(const float* pos, const float* vel, const float* acc, const float* jerk, const float* mass,
                           const int* ticks, int n, int max_level, double dt, int* sched, float* posm, float* velp,
                           nbd_stream_t stream);
/* Acceleration + jerk partial sums of the n_act listed bodies (n_act as schedule reported) under all n of posm / velp. */
int nbd_hblock_force_f32(const float* posm, const float* velp, int n, int n_act, float softening_sq, void* workspace,
                         size_t workspace_bytes, nbd_stream_t stream);
/* Slab sum, corrector with each listed body's own step, new level, ticks[i] = t_next (0 at 2^K), posm[i] = {x1, m}. */
int nbd_hblock_correct_f32(float* pos, float* vel, float* acc, float* jerk, const float* mass, int* ticks, int* levels,
                           int n, int n_act, int max_level, double dt, double eta, float g_const, int* sched, float* posm,
                           void* workspace, size_t workspace_bytes, nbd_stream_t stream);
/* predict + force + correct of one block step (n_act >= 1). */
int nbd_hblock_step_f32(float* pos, float* vel, float* acc, float* jerk, const float* mass, int* ticks, int* levels,
                        int n, int n_act, int max_level, double dt, double eta, float softening_sq, float g_const,
                        int* sched, float* posm, float* velp, void* workspace, size_t workspace_bytes,
                        nbd_stream_t stream);
/* The force alone (tests, profiling): acc_out, jerk_out (n_act,3) of the bodies act[0..n_act) (a device int32 list, any
 * order, no repeats needed) under all n bodies of posm / velp. With n_act = n the sums are nbd_accel_jerk_f32's bits. */
int nbd_accel_jerk_active_f32(const float* posm, const float* velp, int n, const int* act, int n_act,
                              float softening_sq, float g_const, float* acc_out, float* jerk_out, void* workspace,
                              size_t workspace_bytes, nbd_stream_t stream);

/* ---- double-precision block-timestep Hermite (csrc/direct_hermite_block_f64.hip): the block scheme above with the
 * number format of "double-precision Hermite". State, masses, a, j, G, softening_sq, dt, every body's own step constants,
 * the pair arithmetic and all sums are fp64; ticks, levels and sched are the int32 arrays described above, and
 * nbd_hblock_schedule is the scheduler of this mode too. posd / veld: the 32-byte-aligned rows of 4 doubles of
 * nbd_hermite_f64_pack. A block step is nbd_hblock_schedule, then predict, force and correct (or nbd_hblock_step_f64,
 * all three). With every body active the sums are nbd_hermite_step_f64's bits, so max_level = 0 is that step. i == j is
 * dropped by index below softening_sq = 1e-24, otherwise by the term being an exact zero. Workspace:
 * nbd_hblock_f64_workspace_bytes(n), 32-byte aligned; it holds the active list and, 32-byte aligned behind it, the partial
 * sums (6 doubles per listed body and slab). Deterministic (no float atomics, no memsets in a step; the workspace may
 * hold anything on entry). Eager-only, as the fp32 mode. An extension, used only when asked for. */
size_t nbd_hblock_f64_workspace_bytes(int n);
/* nbd_hblock_init_levels from acc, jerk double (n,3). */
int nbd_hblock_init_levels_f64(const double* acc, const double* jerk, int n, double dt, double eta, int max_level,
                               int* ticks, int* levels, int* sched, nbd_stream_t stream);
/* posd = {x_p, m}, veld = {v_p, 0} of every body predicted to t_next = sched[0] over (t_next - ticks[i]) dt / 2^K, the
 * step constants formed in fp64 from that step; zero rows behind n. pos, vel, acc, jerk: double (n,3); mass: double (n). */
int nbd_hblock_predict_f64(const double* pos, const double* vel, const double* acc, const double* jerk,
                           const double* mass, const int* ticks, int n, int max_level, double dt, int* sched,
                           double* posd, double* veld, nbd_stream_t stream);
/* Acceleration + jerk partial sums of the n_act listed bodies (n_act as schedule reported) under all n of posd / veld. */
int nbd_hblock_force_f64(const double* posd, const double* veld, int n, int n_act, double softening_sq, void* workspace,
                         size_t workspace_bytes, nbd_stream_t stream);
/* The slabs in slab order, the corrector with each listed body's own step, new level, ticks[i] = t_next (0 at 2^K),
 * posd[i] = {x1, m}. */
int nbd_hblock_correct_f64(double* pos, double* vel, double* acc, double* jerk, const double* mass, int* ticks,
                           int* levels, int n, int n_act, int max_level, double dt, double eta, double g_const,
                           int* sched, double* posd, void* workspace, size_t workspace_bytes, nbd_stream_t stream);
/* predict + force + correct of one block step (n_act >= 1). */
int nbd_hblock_step_f64(double* pos, double* vel, double* acc, double* jerk, const double* mass, int* ticks, int* levels,
                        int n, int n_act, int max_level, double dt, double eta, double softening_sq, double g_const,
                        int* sched, double* posd, double* veld, void* workspace, size_t workspace_bytes,
                        nbd_stream_t stream);
/* The force alone (tests, profiling): acc_out, jerk_out double (n_act,3) of the bodies act[0..n_act) (a device int32
 * list, any order) under all n bodies of posd / veld, in list order. slabs as in nbd_accel_jerk_f64: 0 for the plan's
 * split of the sources, or an explicit count in [1, 64]; the workspace then needs the list part of
 * nbd_hblock_f64_workspace_bytes(n) (4 bytes per body, n rounded up to a multiple of 8) plus slabs * 6 * n_act doubles.
 * With every body listed the sums are nbd_accel_jerk_f64's bits at the same slab count. */
int nbd_accel_jerk_active_f64(const double* posd, const double* veld, int n, const int* act, int n_act,
                              double softening_sq, double g_const, double* acc_out, double* jerk_out, void* workspace,
                              size_t workspace_bytes, int slabs, nbd_stream_t stream);

/* ---- block-timestep 6th-order Hermite (csrc/direct_hermite_block_f64.hip): "6th-order Hermite" above with the
 * individual power-of-two steps of "double-precision block-timestep Hermite", float64 only. Body i keeps x, v, a, j, s
 * and the crackle c at its last correction tick; ticks, levels and sched are the int32 arrays of the block scheme, the
 * scheduler is nbd_hblock_schedule and the initial levels are nbd_hblock_init_levels_f64's. posd / veld / accd: the
 * 32-byte-aligned rows of 4 doubles of nbd_hermite6_f64_pack. A block step is nbd_hblock_schedule, then predict, force and
 * correct (or nbd_hblock6_step_f64, all three). The new level of a corrected body comes from the generalised Aarseth
 * criterion for p = 6, with eta in the 4th-order convention,
 *   dt_i = (eta^3 (|a1||s1| + |j1|^2) / (|c1||a5| + |a4|^2))^(1/6),
 * a4 (at the end of the step) and a5 from the quintic through (a, j, s) at both ends, c1 the crackle just formed; den = 0
 * allows any step. The level rules are the block scheme's. With every body active the sums are nbd_hermite6_step_f64's
 * bits, so max_level = 0 is that step. i == j is dropped by index below softening_sq = 1e-24, otherwise by the term being
 * an exact zero. Workspace: nbd_hblock6_f64_workspace_bytes(n), 32-byte aligned; it holds the active list and, 32-byte
 * aligned behind it, the partial sums (9 doubles per listed body and slab). Deterministic (no float atomics, no memsets
 * in a step; the workspace may hold anything on entry). Eager-only. Bad arguments are refused before any launch. */
size_t nbd_hblock6_f64_workspace_bytes(int n);
/* posd = {x_p, m}, veld = {v_p, 0}, accd = {a_p, 0} of every body predicted to t_next = sched[0] over
 * (t_next - ticks[i]) dt / 2^K by the Taylor series to the crackle; zero rows behind n. */
int nbd_hblock6_predict_f64(const double* pos, const double* vel, const double* acc, const double* jerk,
                            const double* snap, const double* crackle, const double* mass, const int* ticks, int n,
                            int max_level, double dt, int* sched, double* posd, double* veld, double* accd,
                            nbd_stream_t stream);
/* Acceleration + jerk + snap partial sums of the n_act listed bodies (n_act as schedule reported) under all n sources. */
int nbd_hblock6_force_f64(const double* posd, const double* veld, const double* accd, int n, int n_act,
                          double softening_sq, void* workspace, size_t workspace_bytes, nbd_stream_t stream);
/* The slabs in slab order, the 6th-order corrector and crackle with each listed body's own step, new level,
 * ticks[i] = t_next (0 at 2^K), posd[i] = {x1, m}. */
int nbd_hblock6_correct_f64(double* pos, double* vel, double* acc, double* jerk, double* snap, double* crackle,
                            const double* mass, int* ticks, int* levels, int n, int n_act, int max_level, double dt,
                            double eta, double g_const, int* sched, double* posd, void* workspace,
                            size_t workspace_bytes, nbd_stream_t stream);
/* predict + force + correct of one block step (n_act >= 1). */
int nbd_hblock6_step_f64(double* pos, double* vel, double* acc, double* jerk, double* snap, double* crackle,
                         const double* mass, int* ticks, int* levels, int n, int n_act, int max_level, double dt,
                         double eta, double softening_sq, double g_const, int* sched, double* posd, double* veld,
                         double* accd, void* workspace, size_t workspace_bytes, nbd_stream_t stream);
/* The force alone (tests, profiling): acc_out, jerk_out, snap_out double (n_act,3) of the bodies act[0..n_act) (a device
 * int32 list, any order) under all n bodies of posd / veld / accd, in list order. slabs: 0 for the plan's split of the
 * sources, or an explicit count in [1, 64]; the workspace then needs the list part of nbd_hblock6_f64_workspace_bytes(n)
 * (4 bytes per body, n rounded up to a multiple of 8) plus slabs * 9 * n_act doubles. With every body listed the sums
 * are nbd_accel_jerk_snap_f64's bits at the same slab count. */
int nbd_accel_jerk_snap_active_f64(const double* posd, const double* veld, const double* accd, int n, const int* act,
                                   int n_act, double softening_sq, double g_const, double* acc_out, double* jerk_out,
                                   double* snap_out, void* workspace, size_t workspace_bytes, int slabs,
                                   nbd_stream_t stream);

/* ---- a block step divided over the ranks of a process group (csrc/direct_hermite_block_split_f64.hip), float64, both
 * orders. Every rank holds the whole state, bit for bit the same, and runs nbd_hblock_schedule and the predict entry as
 * they are. A block step with many active bodies is then: nbd_hblock_order_list (the list in ascending body index, alike
 * on every rank); the rows entry for the rank's slice [first, first + count) of the list, which evaluates the slice at its
 * own plan (the slab count of `count` targets), corrects it with each body's own step and writes a header row and one
 * result row per entry into rows_out WITHOUT touching state, levels, ticks or sched; an exchange of the pieces (the
 * caller's: equal pieces of 1 + q rows, rank after rank, into rows_all); and the apply entry on every rank over all n_act
 * entries: the rows scattered into the state, posd[i] = {x1, m}, the new level, ticks[i] = t_next (0 at 2^K), the level
 * histogram, the clamp count, the current tick. List entry p lies in row (p / q) (q + 1) + 1 + p % q of rows_all.
 * A row is NBD_HBLOCK_SPLIT_ROW = 16 doubles (x1 v1 a1 j1, three spare) resp. NBD_HBLOCK6_SPLIT_ROW = 20 (x1 v1 a1 j1 s1
 * c1, one spare); its last double-sized slot holds two int32, {the new level by the block scheme's rules, clamped}. The
 * header row has the same width and starts with int32 {t_next, n_act, first, count}. Spare parts are written as zeros.
 * Apply compares every piece's header with its own record and with the slice that piece should hold (first = min(r q,
 * n_act)); on a mismatch it sets sched[6] (0 otherwise; nbd_hblock_init_levels* clear it) and writes the state all the
 * same. The rows of a slice are the bits nbd_hblock*_correct_f64 would have stored wherever the slab counts of `count` and
 * of n_act targets agree (always for n <= 448). Workspace: nbd_hblock_split_f64_workspace_bytes(n) resp. the hblock6 twin,
 * 32-byte aligned: the ordered list, the ordering's scratch, then a block workspace of the order for the slice. Its head
 * is laid out as nbd_hblock*_f64_workspace_bytes(n)'s, so nbd_hblock_schedule and an un-divided nbd_hblock*_step_f64 run on
 * the same buffer. No float atomics, no memsets; buffers may hold anything on entry. Bad arguments (-1), then a short or
 * misaligned workspace (-2), are refused before any launch. */
#define NBD_HBLOCK_SPLIT_ROW 16
#define NBD_HBLOCK6_SPLIT_ROW 20
size_t nbd_hblock_split_f64_workspace_bytes(int n);
size_t nbd_hblock6_split_f64_workspace_bytes(int n);
/* The list nbd_hblock_schedule has just written, rewritten in ascending body index (two launches, integer work, no
 * readback). sched is read only: t_next, n_act and the cursor fields stay as the scheduler left them. */
int nbd_hblock_order_list(const int* levels, int n, int max_level, int* sched, void* workspace, size_t workspace_bytes,
                          nbd_stream_t stream);
/* The header and the `count` result rows of list entries [first, first + count) into rows_out (32-byte aligned,
 * (1 + count) rows). count = 0: the header only, no force. posd / veld (/ accd): the predict entry's rows. */
int nbd_hblock_split_rows_f64(const double* pos, const double* vel, const double* acc, const double* jerk,
                              const int* levels, int n, int n_act, int first, int count, int max_level, double dt,
                              double eta, double softening_sq, double g_const, const int* sched, const double* posd,
                              const double* veld, double* rows_out, void* workspace, size_t workspace_bytes,
                              nbd_stream_t stream);
int nbd_hblock6_split_rows_f64(const double* pos, const double* vel, const double* acc, const double* jerk,
                               const double* snap, const int* levels, int n, int n_act, int first, int count,
                               int max_level, double dt, double eta, double softening_sq, double g_const,
                               const int* sched, const double* posd, const double* veld, const double* accd,
                               double* rows_out, void* workspace, size_t workspace_bytes, nbd_stream_t stream);
/* All n_act rows of rows_all (world pieces of 1 + q rows; world * q >= n_act) into the state, with the bookkeeping. */
int nbd_hblock_split_apply_f64(const double* rows_all, int world, int q, int n_act, double* pos, double* vel,
                               double* acc, double* jerk, const double* mass, int* ticks, int* levels, int n,
                               int max_level, int* sched, double* posd, void* workspace, size_t workspace_bytes,
                               nbd_stream_t stream);
int nbd_hblock6_split_apply_f64(const double* rows_all, int world, int q, int n_act, double* pos, double* vel,
                                double* acc, double* jerk, double* snap, double* crackle, const double* mass,
                                int* ticks, int* levels, int n, int max_level, int* sched, double* posd,
                                void* workspace, size_t workspace_bytes, nbd_stream_t stream);

/* ---- block-timestep Hermite per scene, 4th and 6th order (csrc/direct_batch_hermite_block_f64.hip): the two block
 * schemes above applied to every scene of an ensemble (offsets, n_scenes as in "batched direct integrator") by ONE
 * schedule and one set of launches per block step, float64 only. All scenes share one tick grid of 2^K ticks per output
 * interval (K = max_level, one value for the batch); scene s's tick is dt_s / 2^K long. The scheduler runs over the bodies
 * of all scenes as one pool; under the block condition a scene gets exactly the active set, at exactly the ticks, it would
 * have alone, so each scene's state, levels and counters are bit-identical to the nbd_hblock_*_f64 / nbd_hblock6_*_f64
 * entries on that scene alone, whatever its companions.
 *   plan    : its own work list in the layout of the float64 batch plan (nbd_batch_hblock_f64_plan for the sizes;
 *             nbd_batch_hblock_f64_plan_fill / nbd_batch_hblock6_f64_plan_fill into a host buffer the caller copies to the
 *             device). The list is STATIC: scene s has max over g in [1, ceil(n_s / 64)] of g * slabs(g) items, slabs(g)
 *             the one-system plan's slab count for g groups of 64 targets under the scene's sources; a block step uses
 *             the first groups * slabs of them for the scene's active count and the rest leave at once.
 *   params  : DEVICE double[NBD_BATCH_HBLOCK_PARAM_ROWS][S], 8-byte aligned, row r of scene s at params[r * S + s]; rows:
 *             G, softening^2, softening, dt, eta.
 *   bsched  : DEVICE int[(S + 1) * NBD_HBLOCK_SCHED_INTS], zero before the first nbd_batch_hblock_init_levels_f64. Record
 *             0 is the ensemble's: [0] t_next, [1] n_act_total, [3] the tick every body has reached, [5] and [8..] the
 *             scheduler's own (finished workgroups, histogram of all levels). Record 1 + s is scene s's: [0] t_next,
 *             [1] the scene's active count of this block step, [2] its cumulative clamp count, [4] and [8..] its list cursor
 *             and level histogram.
 *   counters: DEVICE int64[S][2], zero at the start: the scene's cumulative block steps (those with an active body of
 *             the scene) and pair interactions (sum of n_act_s * n_s). The scheduler adds to them; nothing per scene is
 *             read by the host in a block step.
 *   workspace: nbd_batch_hblock_f64_workspace_bytes / nbd_batch_hblock6_f64_workspace_bytes, 32-byte aligned: the active
 *             lists (int32, n_total rounded up to a multiple of 8; scene s's segment starts at its body offset and holds
 *             scene-local indices) and behind them each scene's partial sums, sized for the largest slabs * n_act any of
 *             its active sets can need (6 resp. 9 doubles per listed body and slab).
 *   posd / veld / accd: the packed rows of the float64 batch entries (nbd_batch_pack_f64, nbd_batch_hermite6_pack_f64).
 * A block step is nbd_batch_hblock_schedule, then predict, force and correct (or nbd_batch_hblock_step_f64 /
 * nbd_batch_hblock6_step_f64, all three). Deterministic: no float atomics, no memsets in a step, the workspace may hold
 * anything on entry. Eager-only: the host reads {t_next, n_act_total} once per block step. The plan and workspace-size
 * entries are host-only. Bad arguments are refused before any launch. */
#define NBD_BATCH_HBLOCK_PARAM_ROWS 5
int nbd_batch_hblock_f64_plan(const int* offsets, int n_scenes, int* n_items, int* rows, size_t* plan_bytes);
int nbd_batch_hblock_f64_plan_fill(const int* offsets, int n_scenes, void* plan, size_t plan_bytes);
int nbd_batch_hblock6_f64_plan_fill(const int* offsets, int n_scenes, void* plan, size_t plan_bytes);
int nbd_batch_hblock_f64_workspace_bytes(const int* offsets, int n_scenes, size_t* bytes);
int nbd_batch_hblock6_f64_workspace_bytes(const int* offsets, int n_scenes, size_t* bytes);
/* ticks = 0 and levels from dt_i = (eta_s / 2) |a| / |j| of the scenes with mask[s] != 0 (mask: DEVICE int[S], or NULL for
 * all), their clamp counts and histograms; then the ensemble's histogram and tick 0. Either order (plan of either). */
int nbd_batch_hblock_init_levels_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes,
                                     const double* acc, const double* jerk, const double* params, int max_level,
                                     const int* mask, int* ticks, int* levels, int* bsched, nbd_stream_t stream);
/* t_next and every scene's active list of the next block step, the scenes' counts and counters. host_sched: NULL, or 4
 * ints of HOST memory that receive record 0's first four after a stream sync. Either order. */
int nbd_batch_hblock_schedule(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const int* levels,
                              int max_level, int* bsched, long long* counters, void* workspace, size_t workspace_bytes,
                              int* host_sched, nbd_stream_t stream);
/* Every body predicted to t_next over (t_next - ticks[i]) dt_s / 2^K into the packed rows; zero rows behind each scene. */
int nbd_batch_hblock_predict_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes,
                                 const double* pos, const double* vel, const double* acc, const double* jerk,
                                 const double* mass, const int* ticks, const double* params, int max_level,
                                 const int* bsched, double* posd, double* veld, nbd_stream_t stream);
int nbd_batch_hblock6_predict_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes,
                                  const double* pos, const double* vel, const double* acc, const double* jerk,
                                  const double* snap, const double* crackle, const double* mass, const int* ticks,
                                  const double* params, int max_level, const int* bsched, double* posd, double* veld,
                                  double* accd, nbd_stream_t stream);
/* The partial sums of every scene's listed bodies under the scene's sources, at the one-system plan of its active count. */
int nbd_batch_hblock_force_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes,
                               const double* posd, const double* veld, const double* params, const int* bsched,
                               void* workspace, size_t workspace_bytes, nbd_stream_t stream);
int nbd_batch_hblock6_force_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes,
                                const double* posd, const double* veld, const double* accd, const double* params,
                                const int* bsched, void* workspace, size_t workspace_bytes, nbd_stream_t stream);
/* The slabs in slab order x G_s, the corrector with each listed body's own step, its new level with eta_s,
 * ticks[i] = t_next (0 at 2^K), posd = {x1, m}; the histograms and the scene's clamp count. */
int nbd_batch_hblock_correct_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, double* pos,
                                 double* vel, double* acc, double* jerk, const double* mass, int* ticks, int* levels,
                                 const double* params, int max_level, int* bsched, double* posd, void* workspace,
                                 size_t workspace_bytes, nbd_stream_t stream);
int nbd_batch_hblock6_correct_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, double* pos,
                                  double* vel, double* acc, double* jerk, double* snap, double* crackle,
                                  const double* mass, int* ticks, int* levels, const double* params, int max_level,
                                  int* bsched, double* posd, void* workspace, size_t workspace_bytes,
                                  nbd_stream_t stream);
/* predict + force + correct of the block step the schedule has just listed. */
int nbd_batch_hblock_step_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, double* pos,
                              double* vel, double* acc, double* jerk, const double* mass, int* ticks, int* levels,
                              const double* params, int max_level, int* bsched, double* posd, double* veld,
                              void* workspace, size_t workspace_bytes, nbd_stream_t stream);
int nbd_batch_hblock6_step_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, double* pos,
                               double* vel, double* acc, double* jerk, double* snap, double* crackle,
                               const double* mass, int* ticks, int* levels, const double* params, int max_level,
                               int* bsched, double* posd, double* veld, double* accd, void* workspace,
                               size_t workspace_bytes, nbd_stream_t stream);

/* ---- backward of the all-pairs acceleration (csrc/direct_grad.hip): the vector-Jacobian product of
 *   a_i = G sum_{j != i} m_j d s^3,  d = x_j - x_i,  s = (|d|^2 + softening_sq)^(-1/2)
 * with a cotangent g = dL/da (n,3). With h_ij = m_i g_j - m_j g_i:
 *   grad_pos[i]  =  G sum_{j != i} [ s^3 h_ij - 3 s^5 d (d . h_ij) ]      (n,3)
 *   grad_mass[i] = -G sum_{j != i}   s^3 (d . g_j)                         (n)
 * An extension (the reference gets these from torch's autograd). The sources are the packed rows of the force entries
 * and, in the same layout, the cotangent rows {gx, gy, gz, 0} with zero rows behind n up to a multiple of 64:
 * nbd_hermite_pack_f32 / nbd_hermite_f64_pack with the cotangent passed as the velocities write exactly this pair.
 * i == j is dropped by index below softening_sq = 1e-24 (the result is the closed form over j != i; torch's autograd gives
 * NaN there), otherwise it is dropped by index in the chunks that hold the targets' own rows and nowhere else (the term
 * is not an exact zero of the arithmetic here). A massless body is a valid source and target. Either of grad_pos /
 * grad_mass may be null (not both).
 * Two launches (partial sums per slab, then the slabs in a fixed order and G applied once); no atomics, no memsets, no
 * host syncs: deterministic with a workspace that may hold anything on entry, and capturable. Refused with
 * NBD_E_BADARG before any launch: n < 0, a null or misaligned pointer (packed rows 16 bytes in fp32 and 32 in fp64; the
 * workspace 16 resp. 8; the outputs their element size), a non-finite softening_sq or g_const. n = 0 succeeds and touches
 * nothing. */
/* Workspace of nbd_accel_vjp_f32: 4 floats per body and slab of the force plan (nbd_accel_plan at n sources, n targets). */
size_t nbd_accel_vjp_workspace_bytes(int n);
int nbd_accel_vjp_f32(const float* posm, const float* cot, int n, float softening_sq, float g_const, float* grad_pos,
                      float* grad_mass, void* workspace, nbd_stream_t stream);
/* float64: slabs = 0 for the split of nbd_hermite_f64_plan, or an explicit slab count in [1, 64] (tests: it sets how many
 * chunks a wave walks). Workspace: 4 doubles per body and slab; 0 for a slab count outside [0, 64]. */
size_t nbd_accel_vjp_f64_workspace_bytes(int n, int slabs);
int nbd_accel_vjp_f64(const double* posd, const double* cotd, int n, double softening_sq, double g_const,
                      double* grad_pos, double* grad_mass, void* workspace, int slabs, nbd_stream_t stream);

/* ------------------------------------------------------------ backward of the Hermite force (direct_hermite_grad.hip)
 * The vector-Jacobian product of (a, j) of nbd_accel_jerk_f32 / nbd_accel_jerk_f64,
 *   j_i = G sum_{j != i} m_j [ s^3 w - 3 s^5 (d . w) d ],  w = v_j - v_i,
 * with the cotangents cota = dL/da and cotj = dL/dj, packed as nbd_accel_vjp_* takes its cotangent ({gx, gy, gz, 0}, zero
 * rows behind n up to a multiple of 64; posm / velp resp. posd / veld are the packed rows of the force entries). With
 * h = m_i cotj_j - m_j cotj_i:
 *   grad_vel[i]  =  G sum_j [ s^3 h - 3 s^5 d (d . h) ]                                                  (n,3)
 *   grad_pos[i]  =  nbd_accel_vjp_*'s grad_pos of cota
 *                 + G sum_j { -3 s^5 [ (h . w) d + (d . h) w + (d . w) h ] + 15 s^7 (d . w)(d . h) d }   (n,3)
 *   grad_mass[i] =  nbd_accel_vjp_*'s grad_mass of cota
 *                 - G sum_j [ s^3 (cotj_j . w) - 3 s^5 (d . w)(d . cotj_j) ]                             (n)
 * Either cotangent may be null (not both): with cotj null grad_pos and grad_mass are nbd_accel_vjp_*'s bits and grad_vel
 * is zeros; with cota null only the new kernels run. With both, the cota part is computed by nbd_accel_vjp_* into the
 * workspace and added last, after G. Any of the three outputs may be null (not all) and is then not written. i == j as
 * for nbd_accel_vjp_*. No atomics, no memsets, no host syncs: deterministic with a workspace that may hold anything on
 * entry, and capturable. Refused with NBD_E_BADARG before any launch: n < 0, a null posm / velp / workspace, a misaligned
 * pointer (rows 16 bytes in fp32 and 32 in fp64; the workspace 16 resp. 8; the outputs their element size), no cotangent,
 * no output, a workspace smaller than nbd_accel_jerk_vjp_*workspace_bytes, slabs outside [0, 64], a non-finite
 * softening_sq or g_const. n = 0 succeeds and touches nothing. */
/* Workspace in floats, S = the slabs of the force plan (nbd_accel_plan at n sources, n targets): 7 S n rounded up to a
 * multiple of 4, then 4 S n (nbd_accel_vjp_f32's own) and 4 n (its results). */
size_t nbd_accel_jerk_vjp_workspace_bytes(int n);
int nbd_accel_jerk_vjp_f32(const float* posm, const float* velp, const float* cota, const float* cotj, int n,
                           float softening_sq, float g_const, float* grad_pos, float* grad_vel, float* grad_mass,
                           void* workspace, size_t workspace_bytes, nbd_stream_t stream);
/* float64: slabs as in nbd_accel_vjp_f64. Workspace: the same sum in doubles; 0 for a slab count outside [0, 64]. */
size_t nbd_accel_jerk_vjp_f64_workspace_bytes(int n, int slabs);
int nbd_accel_jerk_vjp_f64(const double* posd, const double* veld, const double* cota, const double* cotj, int n,
                           double softening_sq, double g_const, double* grad_pos, double* grad_vel, double* grad_mass,
                           void* workspace, size_t workspace_bytes, int slabs, nbd_stream_t stream);

/* ------------------------------------------------------------ surrogate models: graph build
 * Replace the torch_cluster kernels the reference reaches through PyG. Index-exact rule (the
 * reference delegates ties/truncation to torch_cluster; fixed here, see oracle/surrogate_oracle.py):
 * d2 = (dx*dx + dy*dy) + dz*dz in fp32; edges grouped by centre, ascending centre index;
 * edge_index[0] = neighbour j, edge_index[1] = centre i, both int64, row stride = num_edges.
 * seg_lo/seg_hi (both NULL or both given, int32 per node): candidate range = the node's batch
 * segment, replacing PyG's `batch` vector. */

/* knn_graph(pos, k, batch, loop) -- gnn.py:13, datautils.py:36. Per centre the k smallest (d2, j),
 * ties -> lower j, ascending. out_off[i] = first edge slot of centre i (NULL: i * min(k, n - !loop)).
 * k <= 256. */
int nbd_knn_graph_f32(const float* pos, int n, int k, int loop, const int* seg_lo, const int* seg_hi,
                      const int64_t* out_off, int64_t num_edges, int64_t* edge_index, nbd_stream_t stream);

/* The same search with a HINT: hint[i * kk + t], t < kk = min(k, n - 1 (+1 if loop)), are kk distinct
 * neighbours of centre i from an earlier, similar configuration -- in a rollout, the previous step's own
 * edge_index row 0. The largest of their CURRENT distances bounds the kk-th neighbour distance, which saves
 * the first of the two candidate scans; the result is exactly that of nbd_knn_graph_f32 whatever the hint
 * holds (a hint that is not kk distinct valid neighbours is detected and ignored for that centre). hint may
 * alias edge_index (each centre reads its hint before writing its own list). No batch segments / out_off. */
int nbd_knn_graph_hint_f32(const float* pos, int n, int k, int loop, const int* seg_lo, const int* seg_hi,
                           const int64_t* out_off, int64_t num_edges, int64_t* edge_index, const int64_t* hint,
                           nbd_stream_t stream);

/* The radius search of a ROLLOUT (Trainer.evaluate_rollout calls the model once per step on a configuration that
 * has barely moved): same outputs as nbd_radius_search_f32 (no batch segments), exactly, but the O(n^2) scan runs only
 * when some body has moved more than sqrt(moved_sq) since the cached candidate lists were built -- lists of the first
 * wide_cap indices within sqrt(wide_radius_sq) of every centre, kept in `state` together with the reference
 * positions. Every call: one check launch, the (self-skipping) rebuild launches, one re-test launch (one wave per
 * centre over its cached list; a centre whose truncated list holds fewer than max_num_neighbors current hits scans
 * on behind the list). Exact as long as moved <= (wide_radius - radius) / 2; callers leave a margin (graphops.py uses
 * 0.45). state: nbd_radius_cached_state_bytes bytes, 64-byte aligned, ZEROED before its first use and kept by the
 * caller between calls; workspace: nbd_radius_cached_workspace_bytes (scratch). indeg as in nbd_radius_search_f32. */
size_t nbd_radius_cached_state_bytes(int n, int wide_cap);
size_t nbd_radius_cached_workspace_bytes(int n, int wide_cap);
int nbd_radius_cached_search_f32(const float* pos, int n, float radius_sq, float wide_radius_sq, float moved_sq, int loop,
                                 int max_num_neighbors, int wide_cap, void* state, size_t state_bytes, int* nbr, int* deg,
                                 int* last, int* indeg, void* workspace, size_t workspace_bytes, nbd_stream_t stream);

/* The transposed lists (rows = neighbour j, entries = the centres that list j, ascending) straight from the cache of
 * the nbd_radius_cached_search_f32 call that produced `last` on the SAME positions: rowptr = exclusive scan of that
 * call's indeg. Same result as nbd_radius_transpose_lists, without scatter, atomics or per-row sort. */
int nbd_radius_cached_transpose_f32(const float* pos, int n, float radius_sq, int loop, int wide_cap, const void* state,
                                    size_t state_bytes, const int* last, const int* rowptr, int* centres,
                                    nbd_stream_t stream);

/* radius_graph(pos, r, batch, loop, max_num_neighbors) -- contconv.py:225 -- in padded (ELL) form:
 * nbr[i][0..deg[i]) = the first max_num_neighbors indices j (ascending) with d2 < radius_sq
 * (strict), j == i iff loop; last[i] = the largest listed j (-1 if none). No host sync needed. */
int nbd_radius_search_f32(const float* pos, int n, float radius_sq, int loop, int max_num_neighbors,
                          const int* seg_lo, const int* seg_hi, int* nbr, int* deg, int* last, int* indeg,
                          nbd_stream_t stream);

/* radius_graph(loop = False) as torch_cluster 1.6.3 computes it (contconv.py:225 with self_loops = False): search with
 * self as a candidate and max_num_neighbors + 1 slots (the calls here with loop = 1), THEN drop row == col -- a centre
 * with >= max_num_neighbors + 1 lower-indexed hits keeps all max_num_neighbors + 1. This entry point does the drop on
 * lists of `cap` slots per centre: the self entry is removed, deg / last / indeg (optional) follow. (The `loop = 0`
 * mode of the search entry points -- self excluded BEFORE the cap -- is kept for callers that want that rule.) */
int nbd_radius_drop_self_i32(int* nbr, int* deg, int* last, int* indeg, int n, int cap, nbd_stream_t stream);

/* The same search in streaming form (lane = centre, sources broadcast through LDS, the source range cut
 * into slices whose per-centre hit lists are concatenated in index order by a second kernel): identical
 * outputs, ~10x faster at N = 16 384. Needs nbd_radius_search_workspace_bytes(n, max_num_neighbors). */
size_t nbd_radius_search_workspace_bytes(int n, int max_num_neighbors);
int nbd_radius_search_ws_f32(const float* pos, int n, float radius_sq, int loop, int max_num_neighbors,
                             const int* seg_lo, const int* seg_hi, int* nbr, int* deg, int* last, int* indeg,
                             void* workspace, size_t workspace_bytes, nbd_stream_t stream);
/* indeg (optional, int32 [n], zeroed by the call): indeg[j] = number of lists that hold j -- the
 * in-degree the transpose needs, counted with integer atomics while the lists are built.
 *
 * O(E) transpose of the lists (what the ContinuousConv pipeline uses): with rowptr = exclusive scan
 * of indeg, centres[rowptr[j] ..] = the centres c whose list holds j, ascending (scatter through an
 * atomic cursor, then a per-row rank sort: deterministic). cursor: int32 [n] scratch; scratch: int32
 * [>= E] scratch. Same result as the two nbd_radius_transpose_*_f32 scans below. */
int nbd_radius_transpose_lists(const int* nbr, const int* deg, int n, int cap, const int* rowptr, int* cursor,
                               int* scratch, int* centres, nbd_stream_t stream);

/* Transposed adjacency of those capped lists: indeg[j] = number of centres c whose list holds j;
 * after an exclusive scan, centres[rowptr[j] ..] = those c, ascending. This is the grouping
 * ContinuousConv aggregates over (scatter by edge_index[0], contconv.py:82,95-97). */
int nbd_radius_transpose_count_f32(const float* pos, int n, float radius_sq, int loop, const int* seg_lo,
                                   const int* seg_hi, const int* last, int* indeg, nbd_stream_t stream);
int nbd_radius_transpose_fill_f32(const float* pos, int n, float radius_sq, int loop, const int* seg_lo,
                                  const int* seg_hi, const int* last, const int* rowptr, int* centres,
                                  nbd_stream_t stream);

/* Edge list -> CSR grouped by `key` (a row of an int64 edge_index with values in [0, n)): rowptr[n+1],
 * out[e] = the `val` entries of each key in ascending order (duplicates kept). With key = edge_index[0]
 * (sources) and val = edge_index[1] (targets) this is the transposed adjacency that the backward pass of
 * a gather needs so that it is itself a gather with a fixed summation order (the reference's autograd
 * scatters with atomics: gnn.py:170,183 `loss.backward()`). cursor[n], scratch[n_edges]: caller-owned
 * temporaries; *bad_flag (device int) is set to 1 if any key is outside [0, n). */
int nbd_csr_by_key_i64(const int64_t* key, const int64_t* val, int64_t n_edges, int n, int* rowptr, int* cursor,
                       int* scratch, int* out, int* bad_flag, nbd_stream_t stream);

/* ptr[0] = 0, ptr[i+1] = ptr[i] + counts[i]  (int32, n counts -> n+1 entries). */
int nbd_exclusive_scan_i32(const int* counts, int n, int* ptr, nbd_stream_t stream);

/* rowptr[0 .. n] of an edge list whose targets are already in ascending order (knn_graph's output, and the collation of
 * such graphs): rowptr[i] = first edge with tgt >= i. One launch. */
int nbd_rowptr_sorted_i64(const int64_t* tgt, int64_t n_edges, int n, int* rowptr, nbd_stream_t stream);

/* ELL lists -> compact int64 edge_index[2][num_edges] (what radius_graph returns). */
int nbd_ell_to_edge_index(const int* nbr, const int* deg, const int* ptr, int n, int cap, int64_t num_edges,
                          int64_t* edge_index, nbd_stream_t stream);

/* ------------------------------------------------------------ surrogate models: dense blocks */

/* y[r][c] = act( rowscale[r] * sum_k x[r][k] w[c][k]  +  bias_rowscale[r] * bias[c] ),
 * act 0 = identity, 1 = tanh; bias, rowscale, bias_rowscale may be NULL (= 0, 1, 1).
 * torch.nn.Linear layout (w is out x in); ld* are row strides in floats, so inputs/outputs may be
 * column slices of wider buffers (replaces torch.cat). fp32-input MFMA, exact fp32 arithmetic.
 * Used for gnn.py:57-63,75-93,105-114 and contconv.py:92,136-141,206-216. Deterministic. */
int nbd_linear_f32(const float* x, int ldx, const float* w, int ldw, const float* bias, const float* rowscale,
                   const float* bias_rowscale, int act, float* y, int ldy, int n_rows, int n_cols, int k,
                   void* workspace, size_t workspace_bytes, nbd_stream_t stream);
/* Scratch for the split-K path of large products (0 for small ones). Without it the call still
 * succeeds through the un-split kernel. */
size_t nbd_linear_workspace_bytes(int n_rows, int n_cols, int k);

/* EdgeConv aggregation (gnn.py:75-93) after the per-node factoring of its first Linear:
 * pq[i] = [P_i (h) | Q_i (h)], s[i] = aggr_j tanh(P_i + Q_j) over the edges of target i, i.e.
 * src[rowptr[i] .. rowptr[i+1]) (rowptr NULL: exactly fixed_k edges per node, i*fixed_k ..).
 * aggr 0 = sum, 1 = mean (sum / max(count,1)), 2 = max (no edges -> 0). */
int nbd_edgeconv_aggregate_f32(const float* pq, int ldpq, int h, const int* rowptr, const int64_t* src,
                               int fixed_k, int n, int aggr, float* s, int lds, nbd_stream_t stream);

/* EdgeConv with aggr = "max" (PyG's own default; gnn.py:79-93 passes the user's aggr through): the
 * second Linear cannot be hoisted out of a max, so messages are materialised per edge,
 * m[e] = tanh(P_tgt[e] + Q_src[e]) (edges grouped by target), nbd_linear_f32 runs over the E rows and
 * nbd_segment_reduce_f32 reduces each target's rows (mode 0 = sum, 1 = mean, 2 = max; empty -> 0; 3 = product in row
 * order, empty -> 1: torch_scatter's scatter(reduce="mul"), which contconv.py:95-97 reaches with agg="mul"). */
int nbd_edge_messages_f32(const float* pq, int ldpq, int h, const int64_t* src, const int64_t* tgt, int64_t n_edges,
                          float* m, int ldm, nbd_stream_t stream);
int nbd_segment_reduce_f32(const float* m, int ldm, int h, const int* rowptr, int n, int mode, float* out, int ldo,
                           nbd_stream_t stream);

/* torch.nn.LayerNorm over the last dim (gnn.py:146, contconv.py:233); gamma/beta may be NULL. */
int nbd_layernorm_f32(const float* x, int ldx, int c, const float* gamma, const float* beta, float eps, float* y,
                      int ldy, int n, nbd_stream_t stream);

/* LayerNorm + decoder in ONE launch: out = MLP(LayerNorm(x)) (gnn.py:105-114,146-148; contconv.py:206-216,233-234) for
 * c <= 256 channels, n_layers in 1..3 Linears with tanh between them, hidden widths <= 64, last width <= 8
 * (dims[0 .. n_layers], dims[0] = c). w[i] for the hidden layers (i < n_layers - 1) is the TRANSPOSED weight, [in][out]
 * contiguous; w[n_layers - 1] is out x in as torch.nn.Linear holds it; b[i] may be NULL. With hidden layers
 * (n_layers >= 2: fp32 MFMA, 16 rows per wave) the LayerNorm's affine part must come FOLDED into the first Linear --
 * w[0] = (W1 diag(gamma))^T, b[0] = b1 + W1 beta -- and gamma = beta = NULL; with n_layers = 1 gamma / beta are applied
 * here. kick_vel (n x last width,
 * contiguous) non-NULL: kick_vel += kick_c * out in the epilogue (Trainer.step's second half-kick, trainer.py:225-226).
 * nbd_ln_mlp_head_lds_bytes returns 0 for shapes it does not cover (the caller then runs nbd_layernorm_f32 +
 * nbd_linear_f32). Host arrays w / b / dims. */
size_t nbd_ln_mlp_head_lds_bytes(int c, int n_layers, const int* dims);
int nbd_ln_mlp_head_f32(const float* x, int ldx, int c, const float* gamma, const float* beta, float eps, int n_layers,
                        const float* const* w, const float* const* b, const int* dims, float* out, int ldout,
                        float* kick_vel, float kick_c, int n, nbd_stream_t stream);

/* ContinuousConv.forward (contconv.py:80-98) feature-side binning:
 * a_out[n][cell][i] = sum over edges e with edge_index[0][e] == n of
 *      window_e * trilinear_weight_e(cell) * feat[centre_e][i],   cell = (z*D + y)*D + x,
 * window/ball_to_cube/grid_sample(align_corners=True) exactly as contconv.py:30-33,53-78,85-90, so
 * that ContinuousConv = scatter_mean(...) = rowscale * (a_out . filters.reshape(D^3*I, O)).
 * rowptr/centres: CSR by aggregation target (nbd_radius_transpose_*). D <= 10.
 * Rows [node_begin, node_begin + n) are produced into a_out[0 .. n).
 * cell_map (NULL = identity, cells_out ignored): int[D^3], cell -> column block of a_out or -1. ball_to_cube
 * keeps every sample inside |mapped| < tanh(R) (contconv.py:30-33 with the window cut at R, :85-87), so grid
 * points further than that from the cube centre are never touched: their columns are structurally zero and
 * the caller may drop them from a_out AND from the filter matrix (D = 6, R = 1: 160 of 216 cells remain);
 * a_out is then (n, cells_out * in_channels). */
int nbd_contconv_bin_f32(const float* pos, const float* feat, int ldf, int in_channels, const int* rowptr,
                         const int* centres, int node_begin, int n, int filter_resolution, float radius_sq,
                         const int* cell_map, int cells_out, float* a_out, nbd_stream_t stream);

/* One whole EdgeConv layer of GraphModel.forward (gnn.py:75-93,140-148) in ONE launch, one node per
 * wave: s_i = aggr_j tanh(P_i + Q_j); y_i = W2 s_i + beta_i b2 (beta = [deg>0] for mean, deg for sum);
 * then the epilogue. At the reference's sizes the forward pass is launch/latency bound, so this
 * replaces 3 launches per layer (and LayerNorm + head) of the general path; same arithmetic. */
#define NBD_GNN_WRITE_X 0    /* out[i][0..h)   = y_i                      (ldout: column slice ok)    */
#define NBD_GNN_NEXT_PQ 1    /* out[i][0..ep_out) = w_ep y_i + b_ep       (next layer's [P|Q])        */
#define NBD_GNN_FINAL_HEAD 2 /* out[i][0..ep_out) = w_ep LayerNorm([enc_i || y_i]) + b_ep, ep_out<=8 */
#define NBD_GNN_FINAL_LN 3   /* out[i][0..e+h) = LayerNorm([enc_i || y_i])                            */
#define NBD_GNN_NEXT_PQ_FOLDED 4 /* out[i][0..ep_out) = (w_ep W2) S_i + beta_i (w_ep b2) + b_ep: as NEXT_PQ with
                                  * the two mat-vecs folded on the host; the caller passes w_ep := (w_ep W2)^T
                                  * [h][ep_out], b2 := w_ep b2 [ep_out]; w2t is not read                   */
typedef struct nbd_gnn_layer_args {
  const int* rowptr;      /* [n+1] edges grouped by target, or NULL: exactly fixed_k edges per node */
  const int64_t* src;     /* source node j of every edge (edge_index[0])                            */
  int fixed_k, n;
  const float* pq;        /* [n][ldpq] = [P (h) | Q (h)], or NULL: form P/Q from x on the fly       */
  int ldpq;
  const float* x;         /* [n][ldx], first f columns (f <= 8) -- used when pq == NULL             */
  int ldx, f;
  const float* wpq;       /* [2h][f] rows P then Q = [W1a - W1b ; W1b]; bpq [h] = b1                */
  const float* bpq;
  int h, aggr;            /* channels (<= 128); 0 = sum, 1 = mean                                    */
  const float* w2t;       /* [h][h] = W2 TRANSPOSED (in x out: w2t[k][o] = W2[o][k]), b2 [h]          */
  const float* b2;
  int epilogue;           /* NBD_GNN_*                                                               */
  const float* w_ep;      /* NEXT_PQ: [h][ep_out] (TRANSPOSED);  FINAL_HEAD: [ep_out][e+h]          */
  const float* b_ep;
  int ep_out;
  const float* enc;       /* FINAL_*: encoder output [n][ldenc], e columns (e <= 256)                */
  int ldenc, e;
  const float* ln_g;      /* LayerNorm weight / bias [e+h]                                           */
  const float* ln_b;
  float ln_eps;
  float* out;
  int ldout;
  float* kick_vel;        /* FINAL_HEAD only, or NULL: vel[n][ep_out] += kick_c * out_i, the second half-kick of  */
  float kick_c;           /* Trainer.step (trainer.py:225) in the layer's epilogue (multiply, then add)           */
  /* Exponential tables (optional, h <= 64): tanh(P_i + Q_j) = 1 - 2 / (EP_i EQ_j + 1) with EP = 2^(c P), EQ = 2^(c Q),
   * c = 2 log2 e -- one reciprocal per edge and channel instead of an exponential and a reciprocal, the edge loop's
   * bound. epq [n][ldepq] = [EP (h) | EQ (h)] belongs to the SAME P/Q that pq (or x, wpq, bpq) describe: an entry whose
   * |c v| exceeds 100 holds NaN, and a node that meets one is recomputed from pq / x exactly as without tables, so the
   * result never depends on the tables' range. out_epq (NEXT_PQ*): the epilogue also writes the table of its `out`. */
  const float* epq;
  int ldepq;
  float* out_epq;
  int ldout_epq;
  /* Pre-advance (optional; FINAL_HEAD with ep_out == 3, kick_vel set, h == 64 -- NBD_E_UNSUPPORTED otherwise): the
   * leapfrog bookkeeping of a rollout step (trainer.py:217-227) in the epilogue, so that a captured step is the search
   * and the layers only. With vh = adv_vel_half[i] (the half-kicked velocity this step's positions were drifted with),
   * x = adv_pos[i] (those positions: what the search saw) and a = out[i]:
   *   kick_vel[i] = vh + kick_c a        this step's velocity (written, not accumulated)
   *   adv_pos_out[i] = x                 this step's position
   *   adv_vel_half[i] = kick_vel[i] + kick_c a ;  adv_pos[i] = x + adv_dt adv_vel_half[i]    the next step's first half,
   * the new position also into the first three columns of adv_posm[i] (rows of 4: the packed model input). Every product
   * and sum is rounded separately, as nbd_kick_f32 / nbd_kick_drift_f32 round them: the trajectory is bit for bit the one
   * of the separate launches. Only node i's own rows are touched. */
  float* adv_vel_half;
  float* adv_pos;
  float* adv_posm;
  float* adv_pos_out;
  float adv_dt;
} nbd_gnn_layer_args;
int nbd_gnn_layer_f32(const nbd_gnn_layer_args* args, nbd_stream_t stream);

/* GraphModel.predict (gnn.py:205-215: transform_to_graph :11-22, then forward :130-148) as ONE call: the kNN graph of
 * `pos` (k nearest, ascending (d2, j), self excluded unless loop -- nbd_knn_graph_hint_f32's rule) into edge_index
 * [2][n * min(k, n - 1 + loop)], then layers[0 .. n_layers) through nbd_gnn_layer_f32 on that graph (the callee sets
 * each layer's rowptr / src / fixed_k / n). use_hint: edge_index's previous content (an earlier result for a similar
 * configuration, e.g. the previous rollout step) bounds the search; the result does not depend on it. */
#define NBD_GNN_MAX_LAYERS 8
typedef struct nbd_gnn_forward_args {
  const float* pos;       /* [n][3] */
  int n, k, loop, use_hint;
  int64_t* edge_index;    /* [2][n * kk] */
  int n_layers;
  nbd_gnn_layer_args layers[NBD_GNN_MAX_LAYERS];
  void* workspace;        /* optional, nbd_gnn_forward_workspace_bytes(): room for the layers' exponential tables (see  */
  size_t workspace_bytes; /* nbd_gnn_layer_args.epq); with it and h <= 64, first layer formed from x, n <= 8192, the    */
                          /* search kernel also emits the first layer's tables (nbd_knn_graph_hint_pq_f32) and every    */
                          /* NEXT_PQ* epilogue the next one's. NULL / too small: the layers run without tables.         */
} nbd_gnn_forward_args;
size_t nbd_gnn_forward_workspace_bytes(const nbd_gnn_forward_args* args);    /* 0: this configuration uses no tables */
int nbd_gnn_forward_f32(const nbd_gnn_forward_args* args, nbd_stream_t stream);

/* nbd_knn_graph_hint_f32 for ONE un-segmented system (n <= 8192, k <= 200, pos 16-byte aligned; NBD_E_UNSUPPORTED
 * otherwise, nothing launched) whose search kernel, one wave per centre, also writes that centre's row of the first
 * EdgeConv layer's tables: epq[i] = [2^(c P_i) | 2^(c Q_i)], P = wpq[0:h] x_i + bpq, Q = wpq[h:2h] x_i (the fma order of
 * nbd_gnn_layer_f32's on-the-fly form; h <= 64, f <= 8; |c v| > 100 -> NaN, see nbd_gnn_layer_args.epq). Replaces
 * torch_cluster.knn (gnn.py:13) plus the first Linear of gnn.py:140-141 for the rollout. */
typedef struct nbd_knn_pq_args {
  const float* x;         /* [n][ldx], first f columns */
  int ldx, f, h;
  const float* wpq;       /* [2h][f] */
  const float* bpq;       /* [h] */
  float* epq;             /* [n][ldepq] = [EP (h) | EQ (h)] */
  int ldepq;
} nbd_knn_pq_args;
int nbd_knn_graph_hint_pq_f32(const float* pos, int n, int k, int loop, int64_t num_edges, int64_t* edge_index,
                              const int64_t* hint, const nbd_knn_pq_args* pq, nbd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Backward kernels: what `loss.backward()` executes in the reference's training step
 * (gnn.py:163-191 train_batch / train_graph_batch, contconv.py:242-247, driven by trainer.py:60-72)
 * for the layers above. All sums run in a fixed order (row slabs reduced by a second kernel, gathers
 * over sorted adjacency lists): gradients are bit-identical run to run, unlike autograd's atomics.
 * The data gradient of a Linear (dX = g W) is nbd_linear_f32 with the transposed weight.
 * ------------------------------------------------------------------------------------------------- */

/* g = rowscale[n] * dy * act'(y): act 0 = identity, 1 = tanh (1 - y^2); y is the forward OUTPUT;
 * rowscale NULL = 1 (the 1/deg of a mean aggregation, contconv.py:95-97). */
int nbd_act_bwd_f32(const float* dy, int lddy, const float* y, int ldy, int act, const float* rowscale, float* g,
                    int ldg, int n, int c, nbd_stream_t stream);

/* out[c] = sum_n rowweight[n] * x[n][c] (rowweight NULL = 1): bias gradients. */
size_t nbd_colsum_workspace_bytes(int n, int c);
int nbd_colsum_f32(const float* x, int ldx, const float* rowweight, int n, int c, float* out, void* workspace,
                   size_t workspace_bytes, nbd_stream_t stream);

/* dW[m][k] = sum_n g[n][m] * x[n][k]: the weight gradient of Y = X W^T (W is m x k), fp32 MFMA. */
size_t nbd_linear_wgrad_workspace_bytes(int n, int m, int k);
int nbd_linear_wgrad_f32(const float* g, int ldg, const float* x, int ldx, int n, int m, int k, float* dw, int lddw,
                         void* workspace, size_t workspace_bytes, nbd_stream_t stream);
/* The same with the bias gradient in the same launches: db[m] = sum_n rowweight[n] * g[n][m] (rowweight NULL = 1) as one
 * more column of the product (what nbd_colsum_f32 would return; its own summation order, fixed). */
size_t nbd_linear_wgrad_bias_workspace_bytes(int n, int m, int k);
int nbd_linear_wgrad_bias_f32(const float* g, int ldg, const float* x, int ldx, const float* rowweight, int n, int m, int k,
                              float* dw, int lddw, float* db, void* workspace, size_t workspace_bytes, nbd_stream_t stream);

/* Backward of nbd_edgeconv_aggregate_f32 for aggr 0 (sum) / 1 (mean): dpq[n][2h] = [dP | dQ] from ds[n][h].
 * (rowptr | fixed_k, src): the forward's by-target lists; (rowptr_t, tgt_t): the same edges grouped by
 * source (nbd_csr_by_key_i64). */
int nbd_edgeconv_aggregate_bwd_f32(const float* pq, int ldpq, int h, const float* ds, int ldds, const int* rowptr,
                                   const int64_t* src, int fixed_k, const int* rowptr_t, const int* tgt_t, int n,
                                   int aggr, float* dpq, int lddpq, nbd_stream_t stream);

/* torch.nn.BatchNorm1d in TRAINING mode fused with the activation that follows it in the PyG MLP
 * (contconv.py:136-141): y = act(gamma (x - mean) rstd + beta) with the batch mean / biased variance per
 * column, which are also returned (the caller updates running_mean / running_var). n >= 2 as in torch.
 * bwd: dx, dgamma, dbeta from dy (and y when act = tanh). */
size_t nbd_batchnorm_train_workspace_bytes(int n, int c);
int nbd_batchnorm_train_fwd_f32(const float* x, int ldx, int n, int c, const float* gamma, const float* beta, float eps,
                                int act, float* y, int ldy, float* mean, float* var, float* rstd, void* workspace,
                                size_t workspace_bytes, nbd_stream_t stream);
int nbd_batchnorm_train_bwd_f32(const float* x, int ldx, int n, int c, const float* gamma, const float* mean,
                                const float* rstd, int act, const float* y, int ldy, const float* dy, int lddy,
                                float* dx, int lddx, float* dgamma, float* dbeta, void* workspace,
                                size_t workspace_bytes, nbd_stream_t stream);

/* Adjoint of nbd_contconv_bin_f32 with respect to the features: dfeat[c][i] = sum over edges (n <- c) of
 * window * sum_corners t_corner * da[n][cell][i], gathered per SOURCE c over its list of targets n:
 * CSR (rowptr_s, tgt_s) or, with rowptr_s NULL, padded lists tgt_s[c * cap + 0..deg[c]) -- the layout
 * nbd_radius_search_f32 produces. da is (n, cells_out * in_channels) contiguous; cell_map / cells_out as in
 * nbd_contconv_bin_f32. */
int nbd_contconv_bin_bwd_f32(const float* pos, const float* da, int in_channels, const int* rowptr_s, const int* tgt_s,
                             const int* deg, int cap, int n, int filter_resolution, float radius_sq,
                             const int* cell_map, int cells_out, float* dfeat, int lddf, nbd_stream_t stream);

/* Backward of nbd_segment_reduce_f32 mode 2 (max): dm[e][c] = dx[i][c] at the first row e of target i with
 * m[e][c] == x[i][c] (x = the forward output), 0 elsewhere. m may have zero rows for a target. */
int nbd_segment_max_bwd_f32(const float* m, int ldm, int h, const float* x, int ldx, const int* rowptr, int n,
                            const float* dx, int lddx, float* dm, int lddm, nbd_stream_t stream);

/* Backward of nbd_segment_reduce_f32 mode 3 (product): dm[e][c] = dx[i][c] * prod over the OTHER rows e' of target i of
 * m[e'][c] (prefix times suffix: exact when a row holds zeros). */
int nbd_segment_mul_bwd_f32(const float* m, int ldm, int h, const int* rowptr, int n, const float* dx, int lddx,
                            float* dm, int lddm, nbd_stream_t stream);

/* Backward of nbd_layernorm_f32: dx[n][c], dgamma[c], dbeta[c] from x, gamma (NULL = 1) and dy. */
size_t nbd_layernorm_bwd_workspace_bytes(int n, int c);
int nbd_layernorm_bwd_f32(const float* x, int ldx, int c, const float* gamma, float eps, const float* dy, int lddy,
                          float* dx, int lddx, float* dgamma, float* dbeta, int n, void* workspace,
                          size_t workspace_bytes, nbd_stream_t stream);

/* ---- GraphModel's training step with the whole model behind one call per direction (csrc/train_model.hip):
 * forward = gnn.py:130-148 (node encoder MLP or none, message_passing_steps EdgeConv layers with aggr sum / mean in the
 * per-node factored form, LayerNorm over [encoder output | last layer], Linear or MLP decoder), keeping what the
 * backward pass needs in `workspace`; backward = what `loss.backward()` computes for every parameter (gnn.py:170,183,
 * 189), from d loss / d out. Same kernels and summation orders as the per-layer entry points above (bit-reproducible).
 * Weights in torch.nn.Linear layout (out x in, contiguous); w1[l] is the EdgeConv MLP's first Linear (h x 2 F_l),
 * w2[l] its second (h x h). enc_dim[0 .. n_enc] / head_dim[0 .. n_head]: layer widths (tanh between the Linears, none
 * after the last), enc_dim[0] = f, head_dim[0] = encoder output + h. (rowptr | fixed_k, src): edges grouped by target as
 * for nbd_edgeconv_aggregate_f32; (rowptr_t, tgt_t): the same edges grouped by source (nbd_csr_by_key_i64), read by the
 * backward pass only. The same args struct (same workspace) goes to both calls. n = 0: NBD_E_UNSUPPORTED. */
#define NBD_TRAIN_MAX_MLP 8
typedef struct nbd_gnn_train_args {
  int n; const int* rowptr; const int64_t* src; int fixed_k; const int* rowptr_t; const int* tgt_t; int aggr;
  const float* x; int ldx; int f;
  int n_enc; const float* enc_w[NBD_TRAIN_MAX_MLP]; const float* enc_b[NBD_TRAIN_MAX_MLP]; int enc_dim[NBD_TRAIN_MAX_MLP + 1];
  int n_layers; int h;
  const float* w1[NBD_GNN_MAX_LAYERS]; const float* b1[NBD_GNN_MAX_LAYERS];
  const float* w2[NBD_GNN_MAX_LAYERS]; const float* b2[NBD_GNN_MAX_LAYERS];
  const float* ln_g; const float* ln_b; float ln_eps;
  int n_head; const float* head_w[NBD_TRAIN_MAX_MLP]; const float* head_b[NBD_TRAIN_MAX_MLP]; int head_dim[NBD_TRAIN_MAX_MLP + 1];
  float* out; int ldout;
  void* workspace; size_t workspace_bytes;
} nbd_gnn_train_args;
typedef struct nbd_gnn_train_grads {
  float* enc_w[NBD_TRAIN_MAX_MLP]; float* enc_b[NBD_TRAIN_MAX_MLP];
  float* w1[NBD_GNN_MAX_LAYERS]; float* b1[NBD_GNN_MAX_LAYERS]; float* w2[NBD_GNN_MAX_LAYERS]; float* b2[NBD_GNN_MAX_LAYERS];
  float* ln_g; float* ln_b;
  float* head_w[NBD_TRAIN_MAX_MLP]; float* head_b[NBD_TRAIN_MAX_MLP];
} nbd_gnn_train_grads;
size_t nbd_gnn_train_workspace_bytes(const nbd_gnn_train_args* args);
int nbd_gnn_train_forward_f32(const nbd_gnn_train_args* args, nbd_stream_t stream);
int nbd_gnn_train_backward_f32(const nbd_gnn_train_args* args, const float* dout, int lddout,
                               const nbd_gnn_train_grads* grads, nbd_stream_t stream);

/* ---- ContinuousConvModel's training step the same way (contconv.py:218-247; csrc/train_model.hip): node encoder (PyG MLP:
 * Linear -> BatchNorm1d on BATCH statistics (enc_bn = 1; running statistics updated in place when bn_rmean / bn_rvar are
 * given, momentum bn_momentum) -> tanh per hidden layer, plain last Linear; enc_bn = 0: no norm; n_enc = 0: no encoder), the
 * ContinuousConv layers (agg sum / mean, tanh) over the caller's pair lists -- pairs_fwd[l] / pairs_adj[l] from
 * nbd_contconv_pairs_jobs_f32 over the forward (rowptr_fwd, cap_fwd) and adjoint (rowptr_adj, cap_adj) groupings, per
 * layer's filter resolution; pairs_adj[0] may be NULL without an encoder --, LayerNorm over [encoder output | last layer],
 * decoder MLP. filt[l]: the layer's (cells_total, in, out) filters as the module holds them; kept[l] (int64 [n_cells]) /
 * cell_map[l] (int32 [cells_total]) the reachable-cell maps; scale: the 1 / in-degree row scale of a mean aggregation or
 * NULL. Shapes outside nbd_contconv_fused_supported in either direction: workspace_bytes() returns 0 (the caller keeps the
 * per-layer path). Same args struct and workspace for both calls. */
typedef struct nbd_cc_train_args {
  int n; const float* x; int ldx; int in_ch;
  int n_enc; const float* enc_w[NBD_TRAIN_MAX_MLP]; const float* enc_b[NBD_TRAIN_MAX_MLP]; int enc_dim[NBD_TRAIN_MAX_MLP + 1];
  int enc_bn; const float* bn_g[NBD_TRAIN_MAX_MLP]; const float* bn_b[NBD_TRAIN_MAX_MLP]; float bn_eps[NBD_TRAIN_MAX_MLP];
  float* bn_rmean[NBD_TRAIN_MAX_MLP]; float* bn_rvar[NBD_TRAIN_MAX_MLP]; float bn_momentum[NBD_TRAIN_MAX_MLP];
  int n_layers; int cdim;
  const float* filt[NBD_GNN_MAX_LAYERS]; const int64_t* kept[NBD_GNN_MAX_LAYERS]; const int* cell_map[NBD_GNN_MAX_LAYERS];
  int n_cells[NBD_GNN_MAX_LAYERS]; int cells_total[NBD_GNN_MAX_LAYERS];
  const void* pairs_fwd[NBD_GNN_MAX_LAYERS]; const void* pairs_adj[NBD_GNN_MAX_LAYERS];
  const int* rowptr_fwd; int64_t cap_fwd; const int* rowptr_adj; int64_t cap_adj;
  const float* scale;
  const float* ln_g; const float* ln_b; float ln_eps;
  int n_head; const float* head_w[NBD_TRAIN_MAX_MLP]; const float* head_b[NBD_TRAIN_MAX_MLP]; int head_dim[NBD_TRAIN_MAX_MLP + 1];
  float* out; int ldout;
  void* workspace; size_t workspace_bytes;
} nbd_cc_train_args;
typedef struct nbd_cc_train_grads {
  float* enc_w[NBD_TRAIN_MAX_MLP]; float* enc_b[NBD_TRAIN_MAX_MLP]; float* bn_g[NBD_TRAIN_MAX_MLP]; float* bn_b[NBD_TRAIN_MAX_MLP];
  float* filt[NBD_GNN_MAX_LAYERS];
  float* ln_g; float* ln_b;
  float* head_w[NBD_TRAIN_MAX_MLP]; float* head_b[NBD_TRAIN_MAX_MLP];
} nbd_cc_train_grads;
size_t nbd_cc_train_workspace_bytes(const nbd_cc_train_args* args);
int nbd_cc_train_forward_f32(const nbd_cc_train_args* args, nbd_stream_t stream);
int nbd_cc_train_backward_f32(const nbd_cc_train_args* args, const float* dout, int lddout, const nbd_cc_train_grads* grads,
                              nbd_stream_t stream);

/* ---- ContinuousConv.forward (contconv.py:80-98), block-sparse and fused: only the (node, filter cell) blocks
 * some edge touches are multiplied, and the binned features never reach HBM (csrc/contconv_fused.hip).
 * For in_channels % 4 == 0, in_channels <= 128 (nbd_contconv_fused_supported), inference and training alike (the
 * backward pass: nbd_contconv_pairs_jobs_f32 + nbd_contconv_filter_grad_f32 below); other shapes use
 * nbd_contconv_bin_f32 + nbd_linear_f32.
 *
 * nbd_contconv_pairs_f32: the per-(tile of NBD_CC_TILE nodes, cell) lists of (edge corner) pairs {source node,
 *   window * trilinear weight}, grouped by node -- geometry of contconv.py:84-90 evaluated once per edge and
 *   filter resolution. rowptr/centres: edges grouped by aggregation target (edge_index[0]); centres[e] =
 *   edge_index[1]. cell_map (int32 [D^3], -1 = cell dropped) or NULL; n_cells = cells kept. edge_capacity >=
 *   rowptr[n] sizes the lists (host-known bound, e.g. n * max_num_neighbors: no device read-back).
 * nbd_contconv_fused_f32: out[n][:] = act(rowscale[n] * sum_cells A[n][cell] . F[cell]) with
 *   filters_shuffled = the (cell, in, out) filters as nbd_contconv_shuffle_filters_f32 writes them: every element split
 *   into three bf16 terms (hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid), round to nearest even: together
 *   the 24 significant bits of x), in the fragment order of v_mfma_f32_16x16x32_bf16 -- 16-byte quad index
 *   (((cell * ceil(O/16) + cb) * 4 + s) * 3 + u) * 64 + lane holds term u (0 lo, 1 mid, 2 hi) of
 *   F[cell][32 s + 8 (lane >> 4) + e][16 cb + (lane & 15)], e = 0 .. 7; zero beyond I / O (nbd_contconv_filter_floats
 *   counts it in floats: 4 per quad). act: 0 none, 1 tanh. rowscale may be NULL. Deterministic.
 *   Arithmetic: fp32-equivalent. The features are split the same way on chip and the six term products of order <= 2^-16
 *   (all but mid.lo, lo.mid, lo.lo) are accumulated in fp32 on the bf16 matrix pipe; the row error against an fp64
 *   product is no larger than that of the fp32 matrix instruction (tests/test_surrogate_gpu.py holds it to that).
 * Limit: a node with more than 65 535 edges (the pair kernel counts pairs per (node, cell) in 16 bits) is not
 *   processed -- its whole tile of NBD_CC_TILE nodes comes out as NaN, loudly, instead of being summed wrongly. */
int nbd_contconv_fused_supported(int in_channels, int out_channels, int n_cells);
size_t nbd_contconv_pairs_bytes(int n, int64_t edge_capacity, int n_cells);
int nbd_contconv_pairs_f32(const float* pos, const int* rowptr, const int* centres, int n, int64_t edge_capacity,
                           int filter_resolution, float radius_sq, const int* cell_map, int n_cells,
                           void* pair_lists, size_t pair_lists_bytes, nbd_stream_t stream);
/* The pair lists of up to NBD_CC_MAX_RES filter resolutions of ONE graph in a single launch (the layers of a
 * model share the graph and differ in D). Host arrays of n_res entries each. */
int nbd_contconv_pairs_batch_f32(const float* pos, const int* rowptr, const int* centres, int n, int64_t edge_capacity,
                                 float radius_sq, int n_res, const int* filter_resolutions, const int* const* cell_maps,
                                 const int* n_cells, void* const* pair_lists, const size_t* pair_lists_bytes,
                                 nbd_stream_t stream);
/* The general form: up to NBD_CC_MAX_RES pair-list jobs over the same n nodes in ONE launch, each with its own
 * grouping of the edges -- what a training step needs (contconv.py:236-247): the FORWARD lists (rows = aggregation
 * targets edge_index[0], listed nodes = feature sources edge_index[1]) and the ADJOINT lists (rows = feature sources,
 * listed nodes = aggregation targets; adjoint = 1 negates the relative position, which is exact, so an edge gets
 * bit-identical cells and weights in both groupings). With the adjoint lists the gradient with respect to the
 * features is the forward kernel itself: dfeat = nbd_contconv_fused_f32(g, adjoint lists, filters transposed per
 * cell), g = scale * act'(out) * dout. rowptr [n + 1] gives every row's first edge; deg NULL = rows end where the next
 * begins (CSR), else rows are padded (ELL: rowptr[i] = i * cap, deg[i] valid entries -- the radius search's own
 * per-centre lists, unchanged). */
typedef struct nbd_cc_pairs_job {
  const int* rowptr; const int* centres; const int* deg;
  int64_t edge_capacity;
  int filter_resolution; const int* cell_map; int n_cells;
  int adjoint;
  void* pair_lists; size_t pair_lists_bytes;
} nbd_cc_pairs_job;
int nbd_contconv_pairs_jobs_f32(const float* pos, int n, float radius_sq, int n_jobs, const nbd_cc_pairs_job* jobs,
                                nbd_stream_t stream);
/* Gradient of ContinuousConv.forward with respect to `filters` (contconv.py:92-98 under loss.backward()) over the
 * forward pair lists: dfilters[cell][i][o] = sum over the touched (node, cell) blocks of A[node][cell][i] * g[node][o]
 * (cells = the n_cells kept ones, compact order; row-major in x out per cell). fp32 MFMA, the binned matrix is not
 * formed, partial sums per slab of tiles added in fixed order: deterministic. in_channels even, <= 128;
 * out_channels <= 128. */
size_t nbd_contconv_filter_grad_workspace_bytes(int n, int n_cells, int in_channels, int out_channels);
int nbd_contconv_filter_grad_f32(const float* feat, int ldf, int in_channels, const float* g, int ldg, int out_channels,
                                 const int* rowptr, int n, int64_t edge_capacity, const void* pair_lists, int n_cells,
                                 float* dfilters, void* workspace, size_t workspace_bytes, nbd_stream_t stream);
/* The same gradient laid out over the FULL filter grid (cells_total = D^3 cells of in x out; cell_map int32
 * [cells_total] -> compact cell or -1, NULL when every cell is kept): unreachable cells get exact zeros -- the
 * reference's (D, D, D, in, out) `.grad` in one call. workspace >= n_cells * in * out * 4 +
 * nbd_contconv_filter_grad_workspace_bytes(...) bytes. */
int nbd_contconv_filter_grad_full_f32(const float* feat, int ldf, int in_channels, const float* g, int ldg, int out_channels,
                                      const int* rowptr, int n, int64_t edge_capacity, const void* pair_lists, int n_cells,
                                      const int* cell_map, int cells_total, float* dfilters_full, void* workspace,
                                      size_t workspace_bytes, nbd_stream_t stream);
/* filters (cells_total, in, out) row-major -> filters_shuffled, the bf16 x 3 fragment order nbd_contconv_fused_f32 reads
 * (above), over the kept cells kept_cells[0 .. n_cells) (int64 indices into the full grid, ascending). transposed = 1
 * re-lays every cell's filter TRANSPOSED (the operand of the feature gradient: in / out swapped).
 * nbd_contconv_filter_floats floats out (16-byte aligned). Once per weight update. */
int nbd_contconv_shuffle_filters_f32(const float* filters, const int64_t* kept_cells, int n_cells, int in_channels,
                                     int out_channels, int transposed, float* filters_shuffled, nbd_stream_t stream);
/* Byte offsets of the sections of a pair-list buffer (for reports and tests; the layout is otherwise opaque):
 * [0] per-(tile, cell) descriptors, [1] rows, [2] pair records (int2 {source, weight bits}), [3] = [4], [4] step records (int4 per 16-row
 * step), [5] steps per tile (int32 [tiles], tiles = ceil(n / NBD_CC_TILE)), [6] cost per tile (int32 [tiles]),
 * [7] total bytes, [8] float [n]: 1 / max(in-degree, 1), the row scale of a mean aggregation (what
 * nbd_degree_scale_f32 mode 0 returns, written by the pair kernel as a by-product). offsets: 9 entries. The fused
 * kernel multiplies 16 x in x out per step. */
int nbd_contconv_pairs_layout(int n, int64_t edge_capacity, int n_cells, size_t* offsets);
size_t nbd_contconv_fused_workspace_bytes(int n, int n_cells, int out_channels);
size_t nbd_contconv_filter_floats(int in_channels, int out_channels, int n_cells);
int nbd_contconv_fused_f32(const float* feat, int ldf, int in_channels, const int* rowptr, int n, int64_t edge_capacity,
                           const void* pair_lists, const float* filters_shuffled, int n_cells, int out_channels,
                           const float* rowscale, int act, float* out, int ldo, void* workspace,
                           size_t workspace_bytes, nbd_stream_t stream);

/* ContinuousConv's public helpers (contconv.py:30-33 and 53-78), as methods of the drop-in layer:
 * nbd_ball_to_cube_f32: out[i] = r[i] / (|r[i]| + 1e-8) * tanh |r[i]|, r and out (n, 3) row-major.
 * nbd_trilinear_interpolate_f32: out (n, in, out) = the filters (D, D, D, in, out) blended at coords (n, 3) in grid units
 * [0, D - 1] exactly as the reference's F.grid_sample call does it (align_corners = True, zero padding outside the grid,
 * coordinate component 0 along the LAST filter axis). */
int nbd_ball_to_cube_f32(const float* r, int n, float* out, nbd_stream_t stream);
int nbd_trilinear_interpolate_f32(const float* filters, int filter_resolution, int in_channels, int out_channels,
                                  const float* coords, int n, float* out, nbd_stream_t stream);

/* scale[i] from the CSR degree d_i: mode 0 = 1/max(d,1), 1 = d, 2 = (d > 0). */
int nbd_degree_scale_f32(const int* rowptr, int n, int mode, float* scale, nbd_stream_t stream);

/* ------------------------------------------------------------ initial-condition generators on the device
 * generate_disk / generate_spiral (src/galaxify/galaxies.py:54-192, 195-296) AFTER their random draws, in fp64 as
 * upstream. The draws stay on the host: they come from NumPy's legacy global stream and must be consumed in the
 * reference's order for a seed to reproduce its galaxy. generate_disk's O(N^2) enclosed-mass loop (:143-152) is a
 * radix sort by radius + prefix sum + lower-bound search.
 *   u_r, u_z, u_phi   device double[n]: the three vector draws of generate_disk in the reference's order --
 *                     uniform(eps32, 1), uniform(-1, 1), rand()  (:98-112)
 *   rot3x3            device double[9], row-major: positions/velocities are multiplied as row vectors (v @ rot),
 *                     rot = Rx^T Ry^T Rz^T of the Euler angles (:160-186)
 *   offset3_host, initial_vel3_host   HOST double[3] (read at call time)
 *   pos, vel (n,3) and mass (n) device double outputs; body 0 is the central black hole. */
size_t nbd_disk_workspace_bytes(int n);
int nbd_disk_from_draws_f64(const double* u_r, const double* u_z, const double* u_phi, int n, double total_mass,
                            double radial_scale, double height_scale, double g_const, double black_hole_mass,
                            int clockwise, const double* rot3x3, const double* offset3_host,
                            const double* initial_vel3_host, double* pos, double* vel, double* mass, void* workspace,
                            size_t workspace_bytes, nbd_stream_t stream);
/* raw: device double[(n-1)*6], per star {gamma radius, rand, normal z, normal v_R, normal v_phi, normal v_z} in the
 * order the reference draws them (:245-262). */
int nbd_spiral_from_draws_f64(const double* raw, int n, double total_mass, double radial_scale, double height_scale,
                              double g_const, double black_hole_mass, int n_arms, double pitch_angle, double arm_strength,
                              double* pos, double* vel, double* mass, nbd_stream_t stream);

/* ------------------------------------------------------------ dataset CSV rows (host code, no device work)
 * The reference writes one row per particle per state with csv.DictWriter (src/s01-dataset-generation.py:218-241);
 * the nine state columns are numpy.float32 scalars, which the csv module prints with str(): the shortest decimal
 * that reads back as the same fp32, positional for 1e-4 <= |x| < 1e16, d.ddde-XX otherwise.
 *   nbd_format_f32        that string for one value into out24 (>= 24 bytes, not NUL-terminated); returns its length
 *   nbd_format_f32_array  n values into fixed slots of `slot` (>= 24) bytes each, NUL-padded (a numpy 'S<slot>' array)
 *   nbd_csv_format_state  the n rows of one state:  prefix + mass_i + ",x,y,z,vx,vy,vz,ax,ay,az" + suffix, where
 *                         prefix = "scene,scene_type,step,step_time," and suffix = ",u,k\r\n" are the per-state
 *                         constants the caller printed, mass_i = mass_chars[mass_off[i] .. mass_off[i+1]) the per-body
 *                         float64 strings (printed once per scene), pos / vel / acc HOST (n,3) fp32. Returns the bytes
 *                         written, or -1 on a bad argument / cap < nbd_csv_state_bound(...). */
int nbd_format_f32(float x, char* out24);
int nbd_format_f32_array(const float* x, int64_t n, char* out, int slot);
size_t nbd_csv_state_bound(int n, size_t prefix_len, size_t mass_chars, size_t suffix_len);
int64_t nbd_csv_format_state(char* out, size_t cap, const char* prefix, size_t prefix_len, const char* mass_chars,
                             const int32_t* mass_off, const float* pos, const float* vel, const float* acc, int n,
                             const char* suffix, size_t suffix_len);

/* ------------------------------------------------------------ tree-code gravity (csrc/tree_force.hip)
 * The force of nbd_accel_f32 (targets = sources, fp32) in O(N log N): bodies are ordered by the Morton key of their
 * position (21 bits per axis on the bounding cube of all bodies, stable radix sort: equal keys stay in index order) and
 * the hierarchy is implicit over that order: a level-L node holds the sorted bodies [i 8^(L+1), min(n, (i+1) 8^(L+1))),
 * so level 0 has ceil(n/8) nodes of up to 8 bodies and every level above groups 8 consecutive nodes until one is left.
 * A node carries its mass M, centre of mass c, traceless quadrupole Q = sum m (3 d d^T - |d|^2 I) about c and the size
 * s = longest edge of the AABB of its bodies + max-norm of (c - AABB centre); sums in fp64, stored fp32; a node without
 * mass takes c = the mean of its bodies. Targets are walked in groups of 64 consecutive sorted bodies with AABB T; with
 * d the distance from c to T (0 inside), a node is accepted when theta > 0 and s < theta d, else opened into its
 * children, a level-0 node summed body by body (j == i excluded by index, as nbd_accel_f32 does at softening 0). An
 * accepted node adds, with r = c - x_i and u = (|r|^2 + softening_sq)^(-1/2),
 *     M r u^3 - (Q r) u^5 + 2.5 (r^T Q r) r u^7        (the Q terms only when quadrupole != 0),
 * and g_const multiplies the finished sum. theta = 0 is the direct sum in tree order.
 *   nbd_tree_plan             host: levels and nodes over all levels for n bodies (0, 0 for n = 0); n > 2^24 is
 *                             NBD_E_UNSUPPORTED (every entry below refuses it the same way)
 *   nbd_tree_workspace_bytes  bytes of the workspace (the radix sort's scratch included; 0 for n <= 0 or n > 2^24)
 *   nbd_tree_regions          host: the byte offsets, inside that workspace, of the three regions a build leaves and the
 *                             walks read -- the order (n int32: sorted position -> caller's index), the sorted bodies
 *                             (n rounded up to a multiple of 64 rows {x, y, z, m}, zeros behind body n - 1) and the node
 *                             records (3 float4 per node, level 0 first, a level's nodes behind all nodes of the levels
 *                             below it: {c, s}, {M, Qxx, Qxy, Qxz}, {Qyy, Qyz, Qzz, 0}). Each is 256-byte aligned. The
 *                             refusals of nbd_tree_plan, and NBD_E_BADARG for a NULL output; n = 0 gives 0, 0, 0.
 *   nbd_tree_build_f32        keys, sort, sorted bodies and every node into `workspace` (256-byte aligned); order_out[k]
 *                             = the caller's index of the k-th sorted body. pos (n,3), mass (n,).
 *   nbd_tree_accel_f32        the walk over a workspace nbd_tree_build_f32 filled for the same n; acc_out (n,3) in the
 *                             CALLER's order; counters_out NULL or 2 x uint64 on the device = {accepted cells, rejected
 *                             level-0 nodes} summed over the target groups. theta < 0 (or NaN) is NBD_E_BADARG.
 * The potential over the same terms: an accepted node adds
 *     phi_cell = -( M u + 1/2 (r^T Q r) u^5 )           (quadrupole == 0: -M u),
 * whose gradient is the force term above (d u / d x = u^3 r: -grad phi_cell = M u^3 r - (Q r) u^5 + 2.5 (r^T Q r) u^7 r),
 * and a body j of a rejected level-0 node adds -m_j (|d|^2 + softening_sq)^(-1/2). j == i is excluded by index (its term
 * would be m_i / eps, not 0), so a coincident distinct body is kept and gives -inf at softening 0; the zero-mass
 * padding rows behind the last body are excluded too. Pair and cell terms are fp32 and an fp32 sum holds at most 8 of
 * them (the bodies of one level-0 node, 8 consecutive cells); every sum above that is fp64 in a fixed order, and
 * -g_const multiplies the finished sum in fp64. The walk, its lists and its counters are nbd_tree_accel_f32's.
 *   nbd_tree_potential_f32        phi_out (n,) float64 in the CALLER's order; the other arguments, checks and return
 *                                 codes as nbd_tree_accel_f32 (phi_out NULL is NBD_E_BADARG)
 *   nbd_tree_accel_potential_f32  both from one walk: acc_out bit for bit nbd_tree_accel_f32's, phi_out bit for bit
 *                                 nbd_tree_potential_f32's, the same counters
 * Several ranks ("Several ranks"): every rank builds the same tree from the gathered packed rows, walks a
 * contiguous range of the target GROUPS (group g = the sorted bodies [64 g, min(n, 64 g + 64)); ceil(n/64) of them) and
 * places the exchanged rows by `order`. A group's walk reads nothing of another group's, so a row of a ranged walk is
 * bit for bit the row the full walk gives that body, whatever the range.
 *   nbd_tree_build_posm_f32       nbd_tree_build_f32 from packed rows posm (n,4) {x, y, z, m}, 16-byte aligned: order_out
 *                                 and everything the walks read are bit for bit what the two-array build leaves
 *   nbd_tree_accel_groups_f32     the walk of the target groups [group_lo, group_hi) alone: acc_sorted_out
 *                                 ((group_hi - group_lo) 64, 3) in TREE order, row t = sorted body 64 group_lo + t
 *                                 (acc_full[order[k]] == acc_sorted[k - 64 group_lo] bit for bit), rows behind body n - 1
 *                                 written as 0; counters_out = the sums over these groups. 0 <= group_lo <= group_hi <=
 *                                 ceil(n/64), else NBD_E_BADARG; an empty range returns 0, launches nothing and leaves
 *                                 counters_out alone. The workspace is the full walk's (slabs and per-group counters at
 *                                 the global body and group): ranged walks of one workspace run one after another.
 *   nbd_tree_potential_groups_f32, nbd_tree_accel_potential_groups_f32
 *                                 the same for phi_sorted_out ((group_hi - group_lo) 64,) float64 and for both
 *   nbd_tree_scatter_f32          tree order -> a range [lo, hi) of the caller's order: for every sorted position k with
 *                                 lo <= order[k] < hi, acc_out[order[k] - lo] = acc_sorted[k] and phi_out[order[k] - lo] =
 *                                 phi_sorted[k]; acc_sorted (pad64(n),3) or NULL, phi_sorted (pad64(n),) or NULL (both
 *                                 NULL, or 0 <= lo <= hi <= n violated: NBD_E_BADARG), acc_out (hi - lo, 3), phi_out
 *                                 (hi - lo,). One thread per sorted body, no atomics.
 * n = 0 is a no-op. No allocation, memset or synchronisation inside; bit-identical from run to run. */
int nbd_tree_plan(int n, int* levels, int* nodes_total);
size_t nbd_tree_workspace_bytes(int n);
int nbd_tree_regions(int n, size_t* order_off, size_t* posm_off, size_t* nodes_off);
int nbd_tree_build_f32(const float* pos, const float* mass, int n, int* order_out, void* workspace,
                       size_t workspace_bytes, nbd_stream_t stream);
int nbd_tree_accel_f32(const void* workspace, int n, float theta, float softening_sq, float g_const, int quadrupole,
                       float* acc_out, unsigned long long* counters_out, nbd_stream_t stream);
int nbd_tree_potential_f32(const void* workspace, int n, float theta, float softening_sq, float g_const, int quadrupole,
                           double* phi_out, unsigned long long* counters_out, nbd_stream_t stream);
int nbd_tree_accel_potential_f32(const void* workspace, int n, float theta, float softening_sq, float g_const,
                                 int quadrupole, float* acc_out, double* phi_out, unsigned long long* counters_out,
                                 nbd_stream_t stream);
int nbd_tree_build_posm_f32(const float* posm, int n, int* order_out, void* workspace, size_t workspace_bytes,
                            nbd_stream_t stream);
int nbd_tree_accel_groups_f32(const void* workspace, int n, int group_lo, int group_hi, float theta, float softening_sq,
                              float g_const, int quadrupole, float* acc_sorted_out, unsigned long long* counters_out,
                              nbd_stream_t stream);
int nbd_tree_potential_groups_f32(const void* workspace, int n, int group_lo, int group_hi, float theta,
                                  float softening_sq, float g_const, int quadrupole, double* phi_sorted_out,
                                  unsigned long long* counters_out, nbd_stream_t stream);
int nbd_tree_accel_potential_groups_f32(const void* workspace, int n, int group_lo, int group_hi, float theta,
                                        float softening_sq, float g_const, int quadrupole, float* acc_sorted_out,
                                        double* phi_sorted_out, unsigned long long* counters_out, nbd_stream_t stream);
int nbd_tree_scatter_f32(const void* workspace, int n, int lo, int hi, const float* acc_sorted, const double* phi_sorted,
                         float* acc_out, double* phi_out, nbd_stream_t stream);

/* Listed targets ("Block timesteps"): the force on a subset of the bodies, scattered along the curve,
 * against the tree of ALL bodies, without walking every group of 64 that holds one of them.
 *   nbd_tree_active_workspace_bytes  bytes of the workspace of nbd_tree_select_active for n bodies (0 for n <= 0 or
 *                                 n > 2^24), 256-byte aligned: the list (n int32, at byte 0), its count (one int32 at byte
 *                                 4 n rounded up to 256), the flags in tree order and the compaction's scratch
 *   nbd_tree_select_active        list[0 .. n_act) = the sorted positions k, ascending, with flags[order[k]] != 0: the
 *                                 flagged bodies in TREE order. flags (n,) int32 in the caller's order; order is the one
 *                                 nbd_tree_build*_f32 left in `workspace` for the same n. list_out (n int32) and n_act_out
 *                                 (one int32), both on the device; NULL: the active workspace's own. An ordered, stable
 *                                 compaction (hipCUB DeviceSelect): the list is the same from run to run. n_act stays on
 *                                 the device: the caller reads it back. NULL workspace / flags / active workspace or a
 *                                 misaligned one: NBD_E_BADARG; a short active workspace: NBD_E_WORKSPACE.
 *   nbd_tree_accel_active_f32     the walk for the n_act bodies of `list` (the host's copy of what select counted):
 *                                 target group g is the list entries [64 g, min(n_act, 64 g + 64)), one lane each, its
 *                                 box the AABB of those bodies alone; everything else is nbd_tree_accel_f32's walk (j == i
 *                                 excluded by the sorted index). Written: acc_out[order[list[t]]] for t < n_act, acc_out
 *                                 (n,3) in the CALLER's order -- NO other row -- and counters_out, the sums over the
 *                                 listed groups. With list = 0 .. n-1 the groups are the full walk's: acc_out and
 *                                 counters_out equal nbd_tree_accel_f32's bit for bit. An entry outside [0, n) is
 *                                 skipped. n_act = 0 launches nothing and zeroes counters_out if given. n_act > n, a NULL
 *                                 list, or workspace_bytes below nbd_tree_workspace_bytes(n): NBD_E_BADARG, no launch.
 *                                 The slabs and per-group counters are the tree workspace's own, indexed by the active
 *                                 row and group: walks of one workspace run one after another.
 * No allocation or synchronisation inside. */
size_t nbd_tree_active_workspace_bytes(int n);
int nbd_tree_select_active(const void* workspace, int n, const int* flags, int* list_out, int* n_act_out,
                           void* active_workspace, size_t active_workspace_bytes, nbd_stream_t stream);
int nbd_tree_accel_active_f32(const void* workspace, size_t workspace_bytes, int n, const int* list, int n_act, float theta,
                              float softening_sq, float g_const, int quadrupole, float* acc_out,
                              unsigned long long* counters_out, nbd_stream_t stream);

/* ---- block timesteps over the tree force (csrc/tree_block.hip; DESIGN.md K-T, "Block timesteps"): the O(N) stages of
 * a hierarchical kick-drift-kick with individual power-of-two steps. One output interval dt is 2^K ticks, K = max_level
 * in [0, 20]; body i has levels[i] = k_i in [0, K], the step h_i = dt 2^-k_i = d_i = 2^(K - k_i) ticks, and ticks[i] = the
 * tick s_i at which its current step began. sched is a device int[NBD_TBLOCK_SCHED_INTS]: {t_next, n_act, clamped, t_cur,
 * the min being reduced}; zero it once (clamped is cumulative); n_act is written by nbd_tree_select_active, whose
 * n_act_out the caller points at sched + 1, so that ONE copy of sched[0..2) is the readback of a block step.
 * Constants are (float)(0.5 dt 2^-k) and (float)(dt ticks 2^-K), formed in fp64; every update is v += c a or x += c v
 * with product and sum rounded separately (nbd_kick_drift_f32's forms): with K = 0 a step is the shared-step tree
 * leapfrog's bit for bit. The wanted level is the smallest k with (dt 2^-k)^4 (a.a) <= (2 eta softening)^2 in fp64 from the
 * fp32 acceleration (a.a summed x, y, z, products and sums rounded separately); none up to K, or a NaN: K, counted in
 * clamped.
 *   nbd_tblock_init_levels  levels = the wanted ones of acc (n,3), ticks = 0, a new interval
 *   nbd_tblock_open         every body: v += a h_i / 2, ticks = 0, residual (n,3) = 0
 *   nbd_tblock_drift        t_next = min_i (ticks[i] + d_i) (an integer atomic min); every body: x += v (t_next - t_cur)
 *                           dt / 2^K; posm (nbd_posm_padded_len(n), 4) = {x, m}, zeros in the padding. The sum is
 *                           compensated: residual (n,3) fp32 carries the rounding of a position from one block step of
 *                           an interval to the next (y = c v - r; t = x + y; r = (t - x) - y; x = t), because a body at a
 *                           coarse level is drifted up to 2^K times with one velocity and its roundings repeat. With
 *                           r = 0, the first drift of an interval, it is x += c v to the bit.
 *   nbd_tblock_flag         flags[i] = (ticks[i] + d_i == t_next); sched[0] = t_next
 *   nbd_tblock_close        every flagged body: v += a h_i / 2; the level deepens to the wanted one, or rises by ONE if the
 *                           wanted one is coarser and t_next is a multiple of the coarser step's ticks; then, if t_next <
 *                           2^K, v += a h'_i / 2 with the new step and ticks[i] = t_next, else ticks[i] = 0
 * n <= 0 (but nbd_tblock_init_levels: n < 0), max_level outside [0, 20], dt, eta or softening not positive, a NULL array:
 * NBD_E_BADARG. Integer atomics only: the same results from run to run. */
#define NBD_TBLOCK_SCHED_INTS 8
int nbd_tblock_init_levels(const float* acc, int n, double dt, double eta, double softening, int max_level, int* ticks,
                           int* levels, int* sched, nbd_stream_t stream);
int nbd_tblock_open(float* vel, const float* acc, const int* levels, int* ticks, float* residual, int n, int max_level,
                    double dt, int* sched, nbd_stream_t stream);
int nbd_tblock_drift(float* pos, const float* vel, const float* mass, const int* levels, const int* ticks, float* residual,
                     int n, int max_level, double dt, int* sched, float* posm, nbd_stream_t stream);
int nbd_tblock_flag(const int* levels, const int* ticks, int n, int max_level, int* sched, int* flags, nbd_stream_t stream);
int nbd_tblock_close(float* vel, const float* acc, const int* flags, int* levels, int* ticks, int n, int max_level, double dt,
                     double eta, double softening, int* sched, nbd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NBD_H_ */
