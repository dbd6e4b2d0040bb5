/* cavmd.h -- C ABI of the MI355X (gfx950) cavity-MD force engine.
 *
 * This is the drop-in boundary for ONE hot path of muhammadhasyim/cav-hoomd: the per-step
 * cavity force evaluation.  Every entry point names the reference interface it replaces
 * (paths relative to the reference checkout):
 *
 *   reference                                              this library
 *   ----------------------------------------------------   ---------------------------------
 *   struct cavity_force_params  src/CavityForceCompute.h:28-54      cavmd_params / cavmd_make_params
 *   CavityForceComputeGPU ctor (scratch GPUArrays)
 *                               src/CavityForceComputeGPU.cc:31-93  cavmd_create / cavmd_destroy
 *   kernel::gpu_compute_cavity_force(...)
 *                               src/CavityForceComputeGPU.cuh:28-40 cavmd_compute_hoomd
 *   CavityForcePython.set_forces (snapshot-layout arrays)
 *                               src/cavitymd/cavity_force_python.py:65-145
 *                                                                   cavmd_compute_soa
 *   getHarmonicEnergy/getCouplingEnergy/getDipoleSelfEnergy
 *                               src/CavityForceCompute.cc:58-71     cavmd_energies
 *   BussiReservoirThermostat::getRescalingFactorsOne / compute_rescale_factor
 *                               src/BussiReservoirThermostat.h:43-98, 177-225
 *                                                                   cavmd_bussi_step / cavmd_bussi_rescale_factor,
 *                                                                   cavmd_kinetic_energy, cavmd_scale_velocities,
 *                                                                   cavmd_bussi_step_device (the step without a host round trip)
 *   the replica loop (one process, replicas one after the other)
 *                               examples/05_advanced_run.py:1570-1612    cavmd_batch_create / cavmd_batch_compute (all in one launch)
 *   EnergyTracker / CavityModeTracker / DipoleAutocorrelation / AdaptiveTimestepUpdater, per step and replica
 *                               src/cavitymd/analysis.py:425-, 1285-1417, 1424-; src/cavitymd/simulation.py:66-92
 *                                                                   cavmd_recorder_create / cavmd_recorder_record /
 *                                                                   cavmd_recorder_read (a time series in device memory)
 *   EnergyTracker's row (every potential, kinetic and reservoir term, universe_total_energy), per step and replica
 *                               src/cavitymd/analysis.py:425-1046   cavmd_ledger_create / cavmd_ledger_record / cavmd_ledger_read
 *   FieldAutocorrelationTracker, per step and replica
 *                               src/cavitymd/analysis.py:260-418    cavmd_field_recorder_create / cavmd_field_recorder_record /
 *                                                                   cavmd_field_recorder_read (rho(k), F(k,t), references)
 *   hoomd.write.GSD (positions, images and velocities every output period, the initial frame first), per replica
 *                               examples/05_advanced_run.py:1231-1246    cavmd_trajectory_create / cavmd_trajectory_record /
 *                                                                   cavmd_trajectory_read (a ring of frames in device memory)
 *   ElapsedTimeTracker (--runtime) and EnergyTracker's --energy-output-period-ps / --max-energy-output-time, per replica
 *                               src/cavitymd/analysis.py:1230-1259, 692-701   cavmd_runclock_draw_set_end /
 *                                                                   cavmd_runclock_draw_finished / cavmd_runclock_ledger_set_rule /
 *                                                                   cavmd_runclock_field_set_rule
 *                                                                   (decided on the device, by each replica's own clock)
 *   CavityForceCompute::computeForces (the CPU semantics both follow)
 *                               src/CavityForceCompute.cc:134-208   (semantic contract, see below)
 *
 * Conventions
 *   - plain C, plain pointers and sizes; no C++/torch/HOOMD types cross this boundary.
 *   - every function returns an int status: CAVMD_OK (0), a CAVMD_ERR_* code (< 0), or a positive
 *     hipError_t forwarded from the HIP runtime.  Nothing throws across the ABI.
 *   - all particle buffers are DEVICE pointers owned by the caller (HOOMD's GlobalArrays, a torch
 *     tensor, ...).  The library owns only its workspace.  No allocation, no host synchronisation
 *     and no host<->device copy happens inside cavmd_compute_*; they only enqueue kernels on
 *     `stream` (NULL = the null stream, which is what HOOMD-blue 4.x uses), so a caller may
 *     capture them into a hipGraph.  One workspace serves one stream at a time (one force object, as in
 *     the reference).  A workspace that has been captured reads its results (cavmd_result_read,
 *     cavmd_energies) behind a hipDeviceSynchronize instead of the host-visible flag: a replayed kernel
 *     carries the sequence number of its capture, so the flag cannot tell replays apart.
 *     Nor can it keep a history of results (cavmd_result_at answers CAVMD_ERR_INVALID_VALUE from the first captured
 *     evaluation on; see "result history" below).
 *     A graph whose replay ended in CAVMD_ERR_SYNC_TIMEOUT must be captured again before it is replayed (the
 *     library's own recovery -- two launches, wiped hand-off slabs -- does not reach into a captured graph): until then
 *     every replay of it fails at once and as a whole (NaN forces, nothing published; the poison word of
 *     cavmd_persistent_kernel.hpp), it never yields a result.  A graph captured while the single-launch evaluation was in
 *     use keeps that kernel also after a starved-but-REPAIRED replay (valid results): the back-off that moves a workspace
 *     to two launches acts on enqueues, not on replays, so a graph replayed on a GPU that stays oversubscribed can pay the
 *     bounded wait (~0.3 s) on every replay; capture with the tunable "persistent" = 0, or CAVMD_PERSISTENT=0, there.
 *   - Scalar = double (HOOMD's default HOOMD_LONGREAL_SIZE=64 build).
 *
 * Semantic contract (what "the same result as the reference" means here; file:line = reference)
 *   photon      = first index i whose type tag equals L_typeid (src/CavityForceCompute.cc:73-89);
 *                 the tag is the low 32 bits of the bit pattern of pos[i].w (HOOMD __scalar_as_int).
 *   r_i         = pos_i + image_i * (Lx,Ly,Lz), orthorhombic lengths only (:91-111).
 *   d           = sum_{i != photon} charge_i * r_i  (:113-129).  The reference sums left to right;
 *                 this library uses a fixed-shape compensated tree, so d agrees to ~1 ulp with the
 *                 exactly rounded sum, and is bit-reproducible from run to run.
 *   E_h = 1/2 K (q.q) with the 3-D q;  E_c = g (d_xy . q_xy);  E_d = 1/2 (g^2/K)(d_xy . d_xy) (:174-176)
 *   F_i = (-g c_i Dq_x, -g c_i Dq_y, 0, 0) for every particle whose type is not L,
 *         Dq = q_xy + (g/K) d_xy (:183-200);  L-typed particles other than the photon get 0.
 *   F_L = (-K q_x - g d_x, -K q_y - g d_y, -K q_z, 0) (:203-207).
 *   no particle of type L -> all forces 0, all energies 0, not an error (:148-156).
 *   virial / torque are never written (the reference leaves them zero).
 */
#ifndef CAVMD_H_
#define CAVMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define CAVMD_API
#else
#define CAVMD_API __attribute__((visibility("default")))
#endif

#define CAVMD_VERSION_MAJOR 0
#define CAVMD_VERSION_MINOR 2

/* ---- status codes ------------------------------------------------------------------------- */
#define CAVMD_OK 0
#define CAVMD_ERR_INVALID_VALUE (-1) /* null pointer / bad size; mirrors hipErrorInvalidValue at
                                        src/CavityForceComputeGPU.cu:522-528 */
#define CAVMD_ERR_NO_DEVICE (-2)     /* no HIP device visible: the product path never falls back to a CPU */
#define CAVMD_ERR_CAPACITY (-3)      /* N exceeds the capacity the workspace was created for */
#define CAVMD_ERR_BAD_PARAMS (-4)    /* K == 0 or non-finite parameters */
#define CAVMD_ERR_NOT_COMPUTED (-5)  /* results requested before any cavmd_compute_* call */
#define CAVMD_ERR_SYNC_TIMEOUT (-6)  /* a starved single-launch evaluation that could not be completed (see the "persistent"
                                        tunable): that evaluation's forces are NaN.  Returned by cavmd_result_read /
                                        cavmd_energies or by the next cavmd_compute_* call, whichever comes first
                                        (cavmd_result_at returns it for that evaluation without consuming it). */
#define CAVMD_ERR_EXPIRED (-7)       /* the evaluation's slot has been reused: read it sooner or raise "result_history" */

/* ---- layouts (bit-compatible with HOOMD-blue's Scalar4 / int3 in a double-precision build) -- */
typedef struct cavmd_double4
{
    double x, y, z, w;
} cavmd_double4; /* 32 B; pos.w carries the type id in its low 32 bits, force.w is the per-particle PE */

typedef struct cavmd_int3
{
    int32_t x, y, z;
} cavmd_int3; /* 12 B, packed */

/* One POD parameter block shared by host, device and this ABI (the reference defines it twice with
 * different alignment: src/CavityForceCompute.h:28-54 and src/CavityForceComputeGPU.cu:24-30). */
typedef struct cavmd_params
{
    double omegac;   /* cavity frequency, atomic units */
    double couplstr; /* coupling strength g, atomic units */
    double K;        /* spring constant = phmass * omegac^2 */
    double phmass;   /* photon mass */
} cavmd_params;

/* Everything one evaluation produces besides the per-particle forces (192 B, lives in the workspace
 * on the device; cavmd_result_read copies it out). */
typedef struct cavmd_result
{
    double dipole[3];        /* molecular dipole d (photon excluded), all three components */
    double q[3];             /* unwrapped photon position */
    double Dq[2];            /* q_xy + (g/K) d_xy */
    double energy[3];        /* harmonic, coupling, dipole-self */
    double photon_force[3];  /* F_L */
    double dipole_lo[3];     /* low words of the compensated dipole sum (diagnostic) */
    int32_t photon_idx;      /* index of the photon, -1 if there is none */
    int32_t n_photon_typed;  /* how many particles carry type L (the driver enforces exactly 1) */
    uint32_t n_particles;    /* N of the evaluation this result belongs to */
    uint32_t n_partials;     /* partial sums that fed the final reduction (diagnostic) */
    uint64_t sequence;       /* evaluation counter of the workspace */
    double total_dipole[3];  /* sum over ALL particles, L-typed included: what the reference's observable
                                compute_total_dipole_moment (src/cavitymd/analysis.py:18-31) returns */
    double reserved;
} cavmd_result;

typedef struct cavmd_workspace cavmd_workspace; /* opaque */

/* ---- parameters ----------------------------------------------------------------------------- */
/* K = phmass * omegac^2, as cavity_force_params(omegac, couplstr, phmass) at src/CavityForceCompute.h:38-42 */
CAVMD_API cavmd_params cavmd_make_params(double omegac, double couplstr, double phmass);

/* ---- life cycle ----------------------------------------------------------------------------- */
/* Binds a workspace to HIP device `device` (-1 = the current device) sized for up to max_N particles.
 * Replaces the four scratch GPUArrays of CavityForceComputeGPU (src/CavityForceComputeGPU.cc:43-54);
 * unlike them the partial-sum buffer is sized from the launch geometry, never from a constant. */
CAVMD_API int cavmd_create(int device, size_t max_N, cavmd_workspace** out_ws);
CAVMD_API int cavmd_destroy(cavmd_workspace* ws);

/* ---- the hot path --------------------------------------------------------------------------- */
/* HOOMD-native AoS layouts.  Replaces kernel::gpu_compute_cavity_force
 * (src/CavityForceComputeGPU.cuh:28-40): d_force/d_pos/d_charge/d_image keep their meaning, `box`
 * becomes the three orthorhombic lengths box.getL() returns, the four scratch pointers become `ws`.
 * N == 0 is a success that touches nothing (src/CavityForceComputeGPU.cu:530-532).
 * Writes all N entries of d_force (x, y, z and w): no separate memset pass is needed or performed. */
CAVMD_API int cavmd_compute_hoomd(cavmd_workspace* ws,
                                  void* stream,
                                  size_t N,
                                  const cavmd_double4* d_pos,
                                  const double* d_charge,
                                  const cavmd_int3* d_image,
                                  double Lx,
                                  double Ly,
                                  double Lz,
                                  int L_typeid,
                                  const cavmd_params* params,
                                  cavmd_double4* d_force);

/* Snapshot ("local snapshot") layouts used by the hoomd.md.force.Custom surface
 * (src/cavitymd/cavity_force_python.py:72-145): position (N,3) f64, typeid (N,) i32, image (N,3) i32,
 * charge (N,) f64 -> force (N,3) f64 and, if not NULL, potential_energy (N,) f64 (set to 0, as the
 * reference does at :126-131).  Strides are in BYTES between consecutive particles, so the same
 * entry point serves packed arrays (24, 4, 12, 8, 24, 8) and HOOMD's strided views of its Scalar4
 * buffers (32, 32, 12, 8, 32, 32).  Same semantics as cavmd_compute_hoomd (the C++ ones: photon =
 * first particle of type L_typeid, photon excluded from d, L-typed particles get no molecular force). */
CAVMD_API int cavmd_compute_soa(cavmd_workspace* ws,
                                void* stream,
                                size_t N,
                                const double* d_position,
                                size_t position_stride,
                                const int32_t* d_typeid,
                                size_t typeid_stride,
                                const int32_t* d_image,
                                size_t image_stride,
                                const double* d_charge,
                                size_t charge_stride,
                                double Lx,
                                double Ly,
                                double Lz,
                                int L_typeid,
                                const cavmd_params* params,
                                double* d_force,
                                size_t force_stride,
                                double* d_potential_energy,
                                size_t potential_energy_stride);

/* ---- results -------------------------------------------------------------------------------- */
/* The three energy getters of src/CavityForceCompute.cc:58-71 in one call:
 * out[0] = harmonic, out[1] = coupling, out[2] = dipole self-energy.  No copy is enqueued: the kernel that
 * computes the scalars also stores the result block and a sequence flag (system-scope release) into mapped
 * pinned host memory; this call spins until it sees the flag of the last evaluation (or the stream idle).
 * Polled after every evaluation (the reference's EnergyTracker at period 1) it adds ~5 us, not a stream sync. */
CAVMD_API int cavmd_energies(cavmd_workspace* ws, double out[3]);
/* Whole result block (dipole, photon position and force, photon index, ...). */
CAVMD_API int cavmd_result_read(cavmd_workspace* ws, cavmd_result* out);
/* Device address of the result block, for consumers that stay on the GPU (trackers, graphs). */
CAVMD_API int cavmd_result_device_ptr(cavmd_workspace* ws, const cavmd_result** out);

/* ---- result history: read an earlier evaluation without waiting for the newest one -------------------------------- */
/* Every evaluation publishes its result block into its own slot of a ring in mapped pinned host memory (slot
 * sequence % depth, depth = the tunable "result_history", default 64).  A tracker that reads the energies after every step
 * (the reference's EnergyTracker / CavityModeTracker) can then enqueue step k and read step k - 1: the GPU always has the
 * next evaluation queued, and the read costs no wait once that evaluation has published.
 *
 * cavmd_last_sequence: sequence number of the last evaluation enqueued on ws (0 before any; a call with N == 0 consumes
 * none).  No wait.  The n-th evaluation of a workspace has sequence n (cavmd_result.sequence).
 * cavmd_result_at: the result block of evaluation `sequence`, byte for byte what cavmd_result_read returned right after it.
 *   - CAVMD_ERR_NOT_COMPUTED on a workspace that has never evaluated;
 *   - CAVMD_ERR_INVALID_VALUE for sequence 0 or beyond cavmd_last_sequence, and for EVERY sequence once the workspace has
 *     been captured (see below);
 *   - CAVMD_ERR_EXPIRED once depth or more evaluations followed it, or if "result_history" was set after it;
 *   - waits for THAT evaluation only (its slot's flag; the wait also ends once a later evaluation has published or the
 *     stream is idle): never a stream synchronisation, never behind newer evaluations;
 *   - an evaluation that ended without publishing returns an error, never another evaluation's block:
 *     CAVMD_ERR_SYNC_TIMEOUT for a starved single-launch evaluation that could not be completed (the starvation flag is
 *     left for cavmd_result_read / the next cavmd_compute_*, which report it once, as before), a HIP launch failure
 *     otherwise.  Other sequences stay readable.  A starved evaluation that was completed by its last workgroup is valid.
 * cavmd_energies_at: out = its energy[0..2], as cavmd_energies.
 * The synchronous getters above (cavmd_energies, cavmd_result_read, cavmd_result_device_ptr) keep reading the LAST
 * evaluation.  One workspace serves one host thread and one stream: a slot is reused only by an enqueue the caller makes.
 * Graph capture: a captured kernel keeps the sequence and slot it was captured with, so the ring cannot tell its replays
 * apart.  From the first evaluation enqueued into a capture on, the workspace publishes every evaluation (replays and
 * eager ones alike) into one fixed block, read by the synchronous getters behind a device synchronisation as before, and
 * cavmd_result_at / cavmd_energies_at answer CAVMD_ERR_INVALID_VALUE. */
CAVMD_API int cavmd_last_sequence(cavmd_workspace* ws, uint64_t* out);
CAVMD_API int cavmd_result_at(cavmd_workspace* ws, uint64_t sequence, cavmd_result* out);
CAVMD_API int cavmd_energies_at(cavmd_workspace* ws, uint64_t sequence, double out[3]);

/* ---- a batch of independent small systems in ONE launch --------------------------------------------------------------- */
/* The reference's production workload is N = 501 particles run as 500 independent replicas: a sequential loop over replica
 * ids in one process, or one SLURM array task each (examples/05_advanced_run.py:1336-1351, 1570-1612; submit.sh:3).  A caller
 * that holds several of them on one GPU registers their arrays ONCE as a batch and evaluates all of them with one kernel, one
 * 256-thread workgroup per system, instead of one cavmd_compute_hoomd call (one launch, one CU of 256) per replica.
 * Each system's forces and result block are, bit for bit, what cavmd_compute_hoomd gives for that system alone through its
 * single-block kernel (the "small_system_max_n" path): both kernels run the same function.  Systems are independent: no
 * workgroup ever waits for another one inside the launch, hence no starvation and no CAVMD_ERR_SYNC_TIMEOUT on this path. */
typedef struct cavmd_batch_item
{
    const cavmd_double4* d_pos; /* the four arrays of cavmd_compute_hoomd; all DEVICE pointers, same alignments (16/8/4/16) */
    const double* d_charge;
    const cavmd_int3* d_image;
    cavmd_double4* d_force;     /* all N entries are written by every evaluation */
    double Lx, Ly, Lz;
    cavmd_params params;        /* 32 B */
    uint32_t N;                 /* 0 is legal: see below */
    int32_t L_typeid;
    uint64_t reserved[4];       /* must be 0 */
} cavmd_batch_item;             /* 128 B = 32 + 24 + 32 + 8 + 32 */
typedef struct cavmd_batch cavmd_batch; /* opaque; belongs to the workspace it was created from */

#define CAVMD_BATCH_MAX_ITEMS 65536
#define CAVMD_BATCH_MAX_ITEM_N 65536 /* larger systems belong to cavmd_compute_hoomd (crossover measured at 1024) */

/* The per-item validation of cavmd_batch_create / cavmd_batch_set_items, as cavmd_compute_hoomd validates its arguments: host
 * arithmetic only, needs no device.  CAVMD_ERR_INVALID_VALUE for a null item, reserved != 0, a null array (with N > 0) or a
 * misaligned one; CAVMD_ERR_CAPACITY for N > CAVMD_BATCH_MAX_ITEM_N; CAVMD_ERR_BAD_PARAMS for K == 0 or non-finite parameters
 * (with N > 0).  An item with N == 0 is legal and may leave its four arrays NULL: nothing of it is read or written except its
 * result block (all zero, photon_idx = -1, n_particles = 0), so a ragged batch needs no special casing.  What cannot be
 * checked is not: force arrays of two items that overlap, or arrays shorter than N, are the caller's problem. */
CAVMD_API int cavmd_batch_item_check(const cavmd_batch_item* item);
/* Validates the n_items rows in HOST memory (1 .. CAVMD_BATCH_MAX_ITEMS; 0 is CAVMD_ERR_INVALID_VALUE), copies the table to
 * the device of `ws` (set-up time, like cavmd_set_wavevectors: the only copy this path ever makes) and allocates one
 * cavmd_result per item on the device plus a ring of history_depth x n_items 256-byte blocks in mapped pinned host memory.
 * history_depth 2 .. 16384 (else CAVMD_ERR_INVALID_VALUE); CAVMD_ERR_CAPACITY if the ring would exceed 64 MiB.  The batch
 * uses the workspace's device and nothing else of it; destroying the workspace before its batches is an error.  Without a
 * device there is no workspace (cavmd_create: CAVMD_ERR_NO_DEVICE), hence no batch and no CPU fallback. */
CAVMD_API int cavmd_batch_create(cavmd_workspace* ws, size_t n_items, const cavmd_batch_item* h_items, int history_depth,
                                 cavmd_batch** out);
/* Synchronises the stream of the batch's last evaluation (unless that stream is being captured), then frees. */
CAVMD_API int cavmd_batch_destroy(cavmd_batch* b);
/* Rewrites rows first .. first + count - 1 from HOST memory -- how a caller follows a box change or a reallocated array --
 * after synchronising the stream of the last evaluation; validated as in create, nothing is changed if a row is refused.
 * CAVMD_ERR_INVALID_VALUE while that stream is being captured, and for a range outside the batch. */
CAVMD_API int cavmd_batch_set_items(cavmd_batch* b, size_t first, size_t count, const cavmd_batch_item* h_items);
/* Enqueues exactly ONE kernel of n_items workgroups on `stream`: no allocation, no copy, no host wait; may be captured into
 * a hipGraph.  Workgroups start in order of N descending (ties in item order), so the long systems of a ragged batch go
 * first; results stay indexed by item.  The batch counts its own evaluations (the first one is 1): every item's
 * cavmd_result.sequence carries that number.  One batch serves one host thread and one stream at a time. */
CAVMD_API int cavmd_batch_compute(cavmd_batch* b, void* stream);
/* Sequence number of the last evaluation enqueued on b (0 before any).  No wait. */
CAVMD_API int cavmd_batch_last_sequence(cavmd_batch* b, uint64_t* out);
/* Reading follows "result history" above, per item: every workgroup publishes its own block into slot
 * (sequence % history_depth) * n_items + item, after its force stores have been issued.
 * cavmd_batch_results_at / cavmd_batch_energies_at wait for the n_items stamps of THAT evaluation only, never for the stream:
 * out = n_items blocks / 3 * n_items doubles (harmonic, coupling, dipole-self per item).  CAVMD_ERR_NOT_COMPUTED before any
 * evaluation, CAVMD_ERR_INVALID_VALUE for sequence 0 or beyond the last, CAVMD_ERR_EXPIRED once history_depth or more
 * evaluations followed it.  cavmd_batch_results_read = the last evaluation.
 * Graph capture: a replay carries the sequence of its capture, so from the first evaluation enqueued into a capture on the
 * two _at calls answer CAVMD_ERR_INVALID_VALUE, and cavmd_batch_results_read copies the device blocks behind a
 * hipDeviceSynchronize instead of trusting the stamps: the stream a graph is replayed on is not known to the library, so
 * that read waits for EVERY stream of the process on this device, other batches' included (as cavmd_result_read does on a
 * captured workspace).  Forces and the device blocks are right on every replay. */
CAVMD_API int cavmd_batch_results_read(cavmd_batch* b, cavmd_result* out);
CAVMD_API int cavmd_batch_results_at(cavmd_batch* b, uint64_t sequence, cavmd_result* out);
CAVMD_API int cavmd_batch_energies_at(cavmd_batch* b, uint64_t sequence, double* out);
/* Device address of the n_items result blocks (indexed by item), for consumers that stay on the GPU. */
CAVMD_API int cavmd_batch_results_device_ptr(cavmd_batch* b, const cavmd_result** out);

/* ---- several systems of a batch coupled to ONE shared cavity mode, in TWO launches ---------------------------------------- */
/* Collective coupling: one photon coordinate feels the summed dipole of many molecular cells.  The cells are the items of a
 * batch, each with its own box, and the cavity term is the only force that crosses their boundaries.  The reference has no such
 * mode; its formulas (src/CavityForceCompute.cc:166-207) carry over with `dipole` replaced by the sum over the cavity's cells,
 * and a cavity of one cell is the evaluation of cavmd_batch_compute for that item, bit for bit (forces and every field of
 * cavmd_result but sequence and n_partials).
 *
 * A cavity is a set of 1 to CAVMD_SHARED_CAVITY_MAX_MEMBERS items of the object.  Exactly one of them, the carrier, names a
 * photon type (L_typeid >= 0).  The photon is the carrier's first particle of that type, found on the device as
 * cavmd_batch_compute finds it.  Every other member passes L_typeid = -1.
 * With r unwrapped by each member's own box, d_c = sum_i q_i r_i of member c, and D = sum_c d_c:
 *   - The photon is excluded as in the reference.  Further L-typed particles of the carrier are treated as for a single system
 *     (added back to the dipole, zero force).
 *   - E_h = 1/2 K q.q, E_c = g (D_xy . q_xy), E_d = 1/2 (g^2/K) D_xy.D_xy.
 *   - Dq = q_xy + (g/K) D_xy.
 *   - Every non-L particle of every member gets ((-g) q_i) Dq in x and y, with z = 0 and w = 0.
 *   - The photon gets -K q - g D_xy.
 *   - The operator association is the one of a single system (the library evaluates both with the same function).
 *   - If the carrier has no particle of the named type, every force of every member of that cavity is zero and its energies
 *     are zero.  Other cavities are unaffected.
 *   - Members with N == 0 are legal and contribute nothing.
 *
 * Summation order (results are reproducible).  Launch 1 leaves, per member, the un-normalised double-double block total
 * produced by the per-lane order of cavmd_batch_compute: particles base + j*256 + tid, four in flight, then the fixed tree over
 * the 256 threads.  Launch 2 folds the totals of a cavity in ascending item index:
 *   1. Thread t merges members t, t+256, t+512, t+768, in that order, into an identity accumulator.
 *   2. The fixed tree over the 256 threads.
 *   3. The renormalisation hi = fl(hi + lo).
 * The L-typed sums, the photon's index, the count of L-typed particles and the photon row come from the carrier's record alone.
 * Every member's workgroup performs the same fold, so all of them hold identical bits of Dq.  Inside a launch no workgroup
 * waits for another one (no flags, no atomics): the kernel boundary on the stream orders launch 1 before launch 2, hence no
 * starvation and no CAVMD_ERR_SYNC_TIMEOUT on this path.
 *
 * One cavmd_result per item on the device; the recorder, the ledger and the thermalize object take them as they take the
 * batch's (d_result, n_particles == N, photon_idx local to the item):
 *   field                      carrier                                      other member
 *   dipole, dipole_lo          the cavity's D                               its own cell's d_c
 *   total_dipole               D, the L-typed sum joined before rounding    its own cell's d_c
 *   q, Dq                      the cavity's                                 copies of the cavity's
 *   energy, photon_force       the cavity's                                 zero
 *   photon_idx                 local index                                  -1
 *   n_photon_typed             as counted                                   0
 *   n_particles                its N                                        its N
 *   n_partials                 the number of members                        1
 * Summing energy over a cavity's members therefore gives the cavity's.  No member is conserved on its own. */
#define CAVMD_SHARED_CAVITY_MAX_MEMBERS 1024
typedef struct cavmd_shared_cavity_item
{
    const cavmd_double4* d_pos; /* as cavmd_batch_item: all DEVICE pointers, same alignments (16/8/4/16) */
    const double* d_charge;
    const cavmd_int3* d_image;
    cavmd_double4* d_force;     /* all N entries are written by every evaluation */
    double Lx, Ly, Lz;
    cavmd_params params;        /* 32 B; bitwise equal in every member of a cavity */
    uint32_t N;                 /* 0 is legal */
    int32_t L_typeid;           /* >= 0: the carrier of its cavity; -1: another member */
    uint32_t cavity;            /* 0 .. n_cavities - 1 */
    uint32_t reserved0;         /* must be 0 */
    uint64_t reserved[3];       /* must be 0 */
} cavmd_shared_cavity_item;     /* 128 B = 32 + 24 + 32 + 8 + 8 + 24 */
typedef struct cavmd_shared_cavity cavmd_shared_cavity; /* opaque; belongs to the workspace it was created from */

/* The per-row rules of cavmd_batch_item_check (same statuses); host arithmetic only. */
CAVMD_API int cavmd_shared_cavity_item_check(const cavmd_shared_cavity_item* item);
/* Every row, then the rules that cross rows; host arithmetic only, needs no device.  Cavity ids are dense in
 * 0 .. n_cavities - 1 and every cavity has exactly one carrier, else CAVMD_ERR_INVALID_VALUE; `params` are bitwise equal within
 * a cavity, else CAVMD_ERR_BAD_PARAMS; at most CAVMD_SHARED_CAVITY_MAX_MEMBERS members per cavity, else CAVMD_ERR_CAPACITY.
 * n_items 1 .. CAVMD_BATCH_MAX_ITEMS.  *n_cavities (may be NULL) is written for a table that passes. */
CAVMD_API int cavmd_shared_cavity_table_check(size_t n_items, const cavmd_shared_cavity_item* h_items, uint32_t* n_cavities);
/* Validates the table as cavmd_shared_cavity_table_check does, copies it and the member lists derived from it to the device of
 * `ws` and allocates, per item, one cavmd_result, one 128-byte record and four doubles of cell dipole. */
CAVMD_API int cavmd_shared_cavity_create(cavmd_workspace* ws, size_t n_items, const cavmd_shared_cavity_item* h_items,
                                         cavmd_shared_cavity** out);
/* Synchronises the stream of the last evaluation (unless that stream is being captured), then frees. */
CAVMD_API int cavmd_shared_cavity_destroy(cavmd_shared_cavity* c);
/* Rewrites rows first .. first + count - 1 from HOST memory after synchronising the stream of the last evaluation.  The whole
 * table is validated after substitution and nothing is changed if it is refused; membership may change (the member lists are
 * replaced together with the rows, behind a header at a fixed device address, so a graph captured before follows the new
 * table).  CAVMD_ERR_INVALID_VALUE while that stream is being captured, and for a range outside the table. */
CAVMD_API int cavmd_shared_cavity_set_items(cavmd_shared_cavity* c, size_t first, size_t count,
                                            const cavmd_shared_cavity_item* h_items);
/* Enqueues exactly TWO kernels of n_items workgroups each on `stream`: no allocation, no copy, no host wait; may be captured
 * into a hipGraph.  Workgroups start in order of N descending (ties in item order); results stay indexed by item.  The object
 * counts its own evaluations (the first one is 1): every item's cavmd_result.sequence carries that number (a replay carries the
 * number of its capture). */
CAVMD_API int cavmd_shared_cavity_compute(cavmd_shared_cavity* c, void* stream);
/* Sequence number of the last evaluation enqueued (0 before any).  No wait. */
CAVMD_API int cavmd_shared_cavity_last_sequence(cavmd_shared_cavity* c, uint64_t* out);
/* Synchronises `stream`, then copies the n_items device blocks to `out`.  CAVMD_ERR_INVALID_VALUE while `stream` is being
 * captured, CAVMD_ERR_NOT_COMPUTED before any evaluation. */
CAVMD_API int cavmd_shared_cavity_results_read(cavmd_shared_cavity* c, void* stream, cavmd_result* out);
/* Device address of the n_items result blocks (indexed by item), for consumers that stay on the GPU. */
CAVMD_API int cavmd_shared_cavity_results_device_ptr(cavmd_shared_cavity* c, const cavmd_result** out);
/* Device address of the cell dipoles: n_items x 4 doubles (d_c in x, y, z, then 0), each rounded once from its double-double
 * sum; written by launch 1 of every evaluation, also where the cavity has no photon. */
CAVMD_API int cavmd_shared_cavity_cell_dipoles_device_ptr(cavmd_shared_cavity* c, const double** out);
/* The number of cavities of the table, and the item index of a cavity's carrier. */
CAVMD_API int cavmd_shared_cavity_count(cavmd_shared_cavity* c, uint32_t* n_cavities);
CAVMD_API int cavmd_shared_cavity_carrier(cavmd_shared_cavity* c, uint32_t cavity, uint32_t* item);

/* ---- observables next to the force path ------------------------------------------- */
/* Wavevectors for the density field: n_k rows of (kx, ky, kz) in HOST memory; copied into the workspace once.
 * The reference builds them as kmag * generate_fibonacci_sphere(50) (src/cavitymd/analysis.py:296-306). */
CAVMD_API int cavmd_set_wavevectors(cavmd_workspace* ws, size_t n_k, const double* h_wavevectors);
/* rho(k) = sum_j exp(i k . r_j) over the WRAPPED positions of all N particles, for every stored wavevector;
 * replaces compute_density_field (src/cavitymd/analysis.py:34-47), which pulls a CPU snapshot and loops in numpy.
 * d_position + i * position_stride points at particle i's x, y, z (stride 32 for HOOMD's Scalar4 pos, 24 for a
 * packed (N,3) array).  Enqueues two kernels on `stream`; no host synchronisation. */
CAVMD_API int cavmd_density_field(cavmd_workspace* ws, void* stream, size_t N, const double* d_position,
                                  size_t position_stride);
/* Copies the last density field out: h_out[2k] = Re rho(k_k), h_out[2k+1] = Im rho(k_k).  Synchronises the stream. */
CAVMD_API int cavmd_density_field_read(cavmd_workspace* ws, double* h_out);
/* Cavity-mode properties of CavityModeTracker (src/cavitymd/analysis.py:1324-1368) for the photon the last force
 * evaluation found: out = {KE = 1/2 m v.v, harmonic PE, KE + PE, T = (2/3) KE / k_B}; all zero without a photon.
 * d_vel is HOOMD's Scalar4 velocity array (mass in .w); kB in Hartree/K (the reference uses 3.167e-6).
 * Enqueues one tiny kernel on `stream` and spins on its host-visible flag (no copy, no stream synchronisation). */
CAVMD_API int cavmd_cavity_mode(cavmd_workspace* ws, void* stream, const cavmd_double4* d_vel, double kB, double out[4]);

/* S = sum_i |F_i| / m_i over a Scalar4 net-force array and HOOMD's Scalar4 velocity array (mass in .w): the reduction
 * AdaptiveTimestepUpdater performs on the host every step to set dt = sqrt(tol / S) (src/cavitymd/simulation.py:66-92).
 * Enqueues ONE kernel on `stream` (the block that finishes last folds the partials in a fixed order and hands the number to
 * the host through mapped pinned memory); this call spins on its flag: no copy, no stream synchronisation (the caller needs
 * the number to set dt). */
CAVMD_API int cavmd_force_mass_sum(cavmd_workspace* ws, void* stream, size_t N, const cavmd_double4* d_net_force,
                                   const cavmd_double4* d_vel, double* out);

/* ---- Bussi reservoir thermostat step ------------------------------------------------------- */
/* Translational kinetic energy 1/2 sum_j m_j v_j.v_j of a particle group: what BussiReservoirThermostat reads from
 * ComputeThermo (src/BussiReservoirThermostat.h:49-54).  d_vel is HOOMD's Scalar4 velocity array (mass in .w);
 * d_members is a DEVICE array of n_members particle indices (HOOMD's ParticleGroup index list) or NULL for the particles
 * 0 .. n_members-1.  Enqueues ONE kernel on `stream` and spins on its host-visible flag (no copy, no stream
 * synchronisation). */
CAVMD_API int cavmd_kinetic_energy(cavmd_workspace* ws, void* stream, const cavmd_double4* d_vel, const uint32_t* d_members,
                                   size_t n_members, double* out);
/* v_j.xyz *= alpha for the members of the group: what HOOMD's integration method does with the factor the thermostat
 * returns.  Enqueues one kernel; no host synchronisation. */
CAVMD_API int cavmd_scale_velocities(cavmd_workspace* ws, void* stream, cavmd_double4* d_vel, const uint32_t* d_members,
                                     size_t n_members, double alpha);

/* Reservoir accounting of BussiReservoirThermostat (src/BussiReservoirThermostat.h:160-165). */
typedef struct cavmd_bussi_reservoir
{
    double reservoir_translational;     /* cumulative energy handed to the bath by the translational degrees of freedom */
    double reservoir_rotational;
    double instantaneous_translational; /* the same for the last step only */
    double instantaneous_rotational;
} cavmd_bussi_reservoir;

/* The stochastic velocity-rescaling factor alpha of compute_rescale_factor (src/BussiReservoirThermostat.h:177-225),
 * sign rule included, as a pure function of (K, Nf, dt, kT, tau) and the two random variates the reference draws:
 * normal_variate ~ N(0,1), gamma_variate ~ Gamma((Nf - 1) / 2, 1) (ignored unless Nf > 1; drawn only then).
 * Host arithmetic, no GPU needed.  Variate GENERATION is the caller's (HOOMD's RandomGenerator in the reference). */
CAVMD_API int cavmd_bussi_rescale_factor(double K, double degrees_of_freedom, double deltaT, double set_T, double tau,
                                         double normal_variate, double gamma_variate, double* alpha);
/* One thermostat step, as getRescalingFactorsOne (src/BussiReservoirThermostat.h:43-98): factors[0] / [1] = translational /
 * rotational alpha, reservoir counters updated with KE (1 - alpha^2).  variates = {normal_t, gamma_t, normal_r, gamma_r},
 * in the order the reference consumes them.  deltaT == 0 -> {1, 1}, counters untouched;  a non-zero number of degrees
 * of freedom with zero kinetic energy -> CAVMD_ERR_BAD_PARAMS (the reference throws "requires non-zero initial momenta"). */
CAVMD_API int cavmd_bussi_step(cavmd_bussi_reservoir* state, double K_translational, double dof_translational,
                               double K_rotational, double dof_rotational, double deltaT, double set_T, double tau,
                               const double variates[4], double factors[2]);

/* The same translational step ENTIRELY ON THE DEVICE and asynchronous (round 3): kinetic energy of the group -> alpha ->
 * reservoir counters -> velocities *= alpha, as two kernels enqueued on `stream` with no host round trip in between (the
 * first leaves one partial sum per workgroup; every workgroup of the second folds them in a fixed order, evaluates the rule
 * itself and rescales its share; no atomics, no last-workgroup tail).  What
 * getRescalingFactorsOne + the integration method's rescale do per step (src/BussiReservoirThermostat.h:43-98, 177-225) for the
 * translational degrees of freedom; rotational ones stay on the host path above (cavmd_bussi_step).  The rule runs the same
 * source function as cavmd_bussi_rescale_factor (c = exp(-dt / tau) is taken on the host): same bits for the same kinetic energy.
 * deltaT == 0 enqueues nothing (factors 1, counters untouched, :45-48).  Degrees of freedom with zero kinetic energy: the step
 * is refused on the device (alpha = 1, nothing rescaled) and the NEXT cavmd_bussi_device_read returns CAVMD_ERR_BAD_PARAMS once.
 * Not capturable: the variates, c, set_T and dof are kernel arguments, so a step captured into a hipGraph would apply the same
 * random variates on every replay.  While `stream` is being captured the call returns CAVMD_ERR_INVALID_VALUE and enqueues
 * nothing (the step is not counted; the state stays that of the last uncaptured step). */
CAVMD_API int cavmd_bussi_step_device(cavmd_workspace* ws, void* stream, cavmd_double4* d_vel, const uint32_t* d_members,
                                      size_t n_members, double dof_translational, double deltaT, double set_T, double tau,
                                      double normal_variate, double gamma_variate);
typedef struct cavmd_bussi_device_state
{
    double reservoir_translational;     /* cumulative, as cavmd_bussi_reservoir */
    double instantaneous_translational; /* last step */
    double last_alpha;                  /* the factor the last step applied */
    double last_kinetic_energy;         /* the kinetic energy it saw (before rescaling) */
    uint64_t steps;                     /* steps applied since creation / reset */
    uint64_t refused;                   /* steps refused for zero kinetic energy */
} cavmd_bussi_device_state;
/* State after the last enqueued cavmd_bussi_step_device: spins on the flag that step publishes into mapped host memory (no
 * copy, no stream synchronisation; it watches the stream that step was enqueued on); before any step: zeros.
 * CAVMD_ERR_BAD_PARAMS (once) if a step was refused since the last call.  (Steps cannot be captured into a hipGraph: see
 * cavmd_bussi_step_device.) */
CAVMD_API int cavmd_bussi_device_read(cavmd_workspace* ws, cavmd_bussi_device_state* out);
/* reset_reservoir_energy() of the reference's Python class: zero the counters (ordered on `stream`). */
CAVMD_API int cavmd_bussi_device_reset(cavmd_workspace* ws, void* stream);

/* ---- the same translational step for a batch of independent small systems in ONE launch ------------------------------- */
/* The thermostat half of "a batch of independent small systems" above: every replica of the production workload is
 * thermostatted each step (src/BussiReservoirThermostat.h:43-98, 177-225), and cavmd_bussi_step_device costs two launches per
 * system and cannot be captured.  A caller registers the velocity arrays of its B systems ONCE; cavmd_bussi_batch_step then
 * performs the step of all of them with one kernel, one 256-thread workgroup per system (kinetic energy -> alpha -> counters
 * -> velocities *= alpha), and takes the per-step random inputs from a row per item in DEVICE memory, so the launch may be
 * captured into a hipGraph and still applies fresh variates on every replay.
 * Equivalence: per item, velocities and state are bit for bit what cavmd_bussi_step_device gives that item alone with the same
 * inputs, on a device with at least 64 compute units (there the single path sums one tile of 1024 members per workgroup, the
 * order this kernel reproduces).  On a smaller device the batch is still a fixed-order compensated sum (within 2 ulp of the
 * exact kinetic energy), with a tree different from the single path's.  Systems are independent: no workgroup waits for
 * another one, hence no CAVMD_ERR_SYNC_TIMEOUT on this path.  Rotational degrees of freedom stay on the host path
 * (cavmd_bussi_step). */
typedef struct cavmd_bussi_batch_item
{
    cavmd_double4* d_vel;       /* HOOMD Scalar4 velocities, mass in .w; DEVICE pointer, 16-byte aligned */
    const uint32_t* d_members;  /* device index list of the thermostatted group, or NULL = 0 .. n_members-1 */
    uint32_t n_members;         /* 0 is legal: the item is never touched or counted; <= CAVMD_BATCH_MAX_ITEM_N */
    uint32_t reserved0;         /* must be 0 */
    double dof_translational;
    uint64_t reserved[4];       /* must be 0 */
} cavmd_bussi_batch_item;       /* 64 B */
typedef struct cavmd_bussi_batch_input /* one row per item, in DEVICE memory, owned by the caller */
{
    double normal_variate;      /* as cavmd_bussi_step_device */
    double gamma_variate;
    double c;                   /* exp(-deltaT / tau), 0 for tau == 0 */
    double set_T;
    uint64_t skip;              /* != 0: deltaT == 0, velocities and counters of this item untouched */
    uint64_t reserved[3];
} cavmd_bussi_batch_input;      /* 64 B */
typedef struct cavmd_bussi_batch cavmd_bussi_batch; /* opaque; belongs to the workspace it was created from */

/* Per-item validation of create / set_items; host arithmetic only, needs no device.  CAVMD_ERR_INVALID_VALUE for a null item,
 * a null d_vel (with n_members > 0), a d_vel not 16-byte or a d_members not 4-byte aligned, reserved != 0, a negative or
 * non-finite dof_translational; CAVMD_ERR_CAPACITY for n_members > CAVMD_BATCH_MAX_ITEM_N. */
CAVMD_API int cavmd_bussi_batch_item_check(const cavmd_bussi_batch_item* item);
/* Fills one input row on the HOST from the arguments of cavmd_bussi_step_device, with the expression that call uses:
 * c = tau != 0 ? exp(-deltaT / tau) : 0, skip = (deltaT == 0).  Needs no device.  The caller copies rows to its device array. */
CAVMD_API int cavmd_bussi_batch_input_make(double deltaT, double set_T, double tau, double normal_variate,
                                           double gamma_variate, cavmd_bussi_batch_input* row);
/* Validates the n_items rows in HOST memory (1 .. CAVMD_BATCH_MAX_ITEMS), copies the table to the device of `ws` (set-up
 * time) and allocates one state per item on the device plus one 64-byte block per item in mapped pinned host memory.  All
 * counters start at zero.  Destroying the workspace before its thermostat batches is an error: cavmd_destroy answers
 * CAVMD_ERR_INVALID_VALUE and frees nothing while one is alive.  Without a device there is no workspace, hence no batch. */
CAVMD_API int cavmd_bussi_batch_create(cavmd_workspace* ws, size_t n_items, const cavmd_bussi_batch_item* h_items,
                                       cavmd_bussi_batch** out);
/* Synchronises the stream of the batch's last step (unless that stream is being captured), then frees. */
CAVMD_API int cavmd_bussi_batch_destroy(cavmd_bussi_batch* b);
/* Rewrites rows first .. first + count - 1 from HOST memory (a reallocated velocity array, another group) after synchronising
 * the stream of the last step; nothing is changed if a row is refused; the items' counters are kept.
 * CAVMD_ERR_INVALID_VALUE while that stream is being captured, and for a range outside the batch. */
CAVMD_API int cavmd_bussi_batch_set_items(cavmd_bussi_batch* b, size_t first, size_t count,
                                          const cavmd_bussi_batch_item* h_items);
/* Enqueues exactly ONE kernel of n_items workgroups on `stream`: no allocation, no copy, no host wait.  d_inputs: n_items rows
 * in DEVICE memory (CAVMD_ERR_INVALID_VALUE if null or not 8-byte aligned), read by the kernel when it RUNS.  May be captured
 * into a hipGraph: a replay reads whatever d_inputs holds at that moment, so the caller refreshes that buffer, in stream
 * order, between replays; the pointer itself is frozen at capture.  An item whose row has skip != 0, and an item with
 * n_members == 0, is left alone: velocities and counters untouched, nothing counted.  Workgroups start in order of n_members
 * descending (ties in item order); states stay indexed by item.  One batch serves one host thread and one stream at a time. */
CAVMD_API int cavmd_bussi_batch_step(cavmd_bussi_batch* b, void* stream, const cavmd_bussi_batch_input* d_inputs);
/* Number of steps enqueued on b (0 before any).  No wait. */
CAVMD_API int cavmd_bussi_batch_last_sequence(cavmd_bussi_batch* b, uint64_t* out);
/* out = n_items states after the last enqueued step: waits for the n_items stamps of THAT step only (every workgroup stamps
 * its item's host block after its velocity stores have been issued; a skipped item is stamped too and keeps its earlier
 * state), or for that step's stream to be idle; never a stream synchronisation.  Before any step: zeros (after a
 * cavmd_snapshot_bussi_batch_load: the loaded states, copied from the device).
 * CAVMD_ERR_BAD_PARAMS, ONCE, if a step of any item was refused for zero kinetic energy since the last read; `out` is filled
 * all the same (per item: `refused`).  Once the batch has seen a capturing stream the stamps cannot be trusted (a replay
 * carries the sequence of its capture): the read then copies the device states behind a hipDeviceSynchronize, as
 * cavmd_batch_results_read does. */
CAVMD_API int cavmd_bussi_batch_read(cavmd_bussi_batch* b, cavmd_bussi_device_state* out);
/* Zero all counters of all items (ordered on `stream`). */
CAVMD_API int cavmd_bussi_batch_reset(cavmd_bussi_batch* b, void* stream);
/* Device address of the n_items states (indexed by item; six 8-byte words each: reservoir, instantaneous, alpha, kinetic
 * energy, steps, refused -- the layout of cavmd_bussi_device_state), for consumers that stay on the GPU. */
CAVMD_API int cavmd_bussi_batch_state_device_ptr(cavmd_bussi_batch* b, const cavmd_bussi_device_state** out);

/* ---- per-step observables of a batch, recorded on the device: the third kernel of the batched step -------------------- */
/* What the reference's trackers write every step for every replica -- EnergyTracker (src/cavitymd/analysis.py:425-),
 * CavityModeTracker (:1285-1417), DipoleAutocorrelation (:1424-) and the reduction of AdaptiveTimestepUpdater
 * (src/cavitymd/simulation.py:66-92) -- as ONE launch for all systems that appends one 128-byte record per system to a time
 * series kept in DEVICE memory.  The write position is kept on the device too, so a hipGraph replay appends a NEW row each
 * time: the series is how a captured {cavmd_batch_compute, cavmd_recorder_record, cavmd_bussi_batch_step} loop is observed
 * (cavmd_batch_results_at / cavmd_batch_energies_at cannot tell replays apart, see above).  The host reads the series when it
 * likes -- every few thousand steps, or once at the end -- behind a synchronisation of the stream it names; nothing is mapped,
 * nothing is polled.  Systems are independent: no workgroup waits for another one, hence no CAVMD_ERR_SYNC_TIMEOUT here.
 * Equivalences, per item and recorded row, bit for bit:
 *   - energy, total_dipole, q, eval_sequence: the bytes of the cavmd_result block d_result points at when the kernel runs;
 *   - cavity_kinetic, cavity_temperature: cavmd_cavity_mode's out[0], out[3] for that system alone, and
 *     cavity_kinetic + energy[0] is its out[2] (one IEEE addition on either side);
 *   - kinetic_energy = cavmd_kinetic_energy, force_mass_sum = cavmd_force_mass_sum for that item alone, on a device with at
 *     least 64 compute units (there the single paths sum one tile of 1024 entries per workgroup, the order this kernel
 *     reproduces; same condition and reason as for cavmd_bussi_batch_step).  On a smaller device they are still fixed-order
 *     compensated sums within 2 ulp of the exact value, with a tree different from the single paths'. */
typedef struct cavmd_record              /* 128 B, one per item and recorded call */
{
    uint64_t call;            /* 1-based index of the cavmd_recorder_record call (of this item) that wrote the row */
    uint64_t eval_sequence;   /* cavmd_result.sequence of the block it read (frozen under replay: diagnostic only) */
    double energy[3];         /* harmonic, coupling, dipole-self: bytes of cavmd_result.energy */
    double total_dipole[3];   /* bytes of cavmd_result.total_dipole (DipoleAutocorrelation's observable) */
    double q[3];              /* bytes of cavmd_result.q */
    double cavity_kinetic;    /* CavityModeTracker: KE; its PE is energy[0], its total is cavity_kinetic + energy[0] */
    double cavity_temperature;
    double kinetic_energy;    /* of the item's group, as cavmd_kinetic_energy */
    double force_mass_sum;    /* as cavmd_force_mass_sum; dt = sqrt(tol / S) stays the caller's, or is taken on the device
                                 by cavmd_draw_fill (the section "the step inputs of a batch, drawn on the device") */
    double reserved;          /* 0 */
} cavmd_record;

typedef struct cavmd_recorder_item       /* 64 B; all pointers DEVICE pointers */
{
    const cavmd_result* d_result;        /* required: e.g. cavmd_batch_results_device_ptr + item */
    const cavmd_double4* d_vel;          /* Scalar4 velocities, mass in .w, of the system d_result belongs to (the photon's
                                            entry is read at its photon_idx); NULL: the three velocity columns are 0 */
    const cavmd_double4* d_net_force;    /* Scalar4 net force; NULL (or d_vel NULL): force_mass_sum is 0 */
    const uint32_t* d_members;           /* group of kinetic_energy, or NULL = 0 .. n_members-1 */
    uint32_t N;                          /* particles covered by force_mass_sum; <= CAVMD_BATCH_MAX_ITEM_N */
    uint32_t n_members;                  /* <= CAVMD_BATCH_MAX_ITEM_N; 0 is legal (kinetic_energy 0) */
    uint64_t reserved[3];                /* must be 0 */
} cavmd_recorder_item;
typedef struct cavmd_recorder cavmd_recorder; /* opaque; belongs to the workspace it was created from */

/* Per-item validation of create / set_items; host arithmetic only, needs no device.  CAVMD_ERR_INVALID_VALUE for a null item,
 * a null d_result, a d_result / d_vel / d_net_force not 16-byte or a d_members not 4-byte aligned, reserved != 0;
 * CAVMD_ERR_CAPACITY for N or n_members above CAVMD_BATCH_MAX_ITEM_N. */
CAVMD_API int cavmd_recorder_item_check(const cavmd_recorder_item* item);
/* Validates the n_items rows in HOST memory (1 .. CAVMD_BATCH_MAX_ITEMS), copies the table to the device of `ws` (set-up time)
 * and allocates n_items x capacity records plus the per-item counters in device memory, all zero.  Every `period`-th call of
 * cavmd_recorder_record writes a row (period 1: every call); an item keeps its last `capacity` rows.  capacity >= 1,
 * period >= 1, kB > 0 and finite (Hartree/K, as cavmd_cavity_mode), else CAVMD_ERR_INVALID_VALUE; CAVMD_ERR_CAPACITY if the
 * series would exceed 1 GiB.  cavmd_destroy answers CAVMD_ERR_INVALID_VALUE and frees nothing while a recorder of the
 * workspace is alive.  Without a device there is no workspace, hence no recorder. */
CAVMD_API int cavmd_recorder_create(cavmd_workspace* ws, size_t n_items, const cavmd_recorder_item* h_items, size_t capacity,
                                    uint64_t period, double kB, cavmd_recorder** out);
/* Synchronises the stream of the last cavmd_recorder_record call (unless that stream is being captured), then frees. */
CAVMD_API int cavmd_recorder_destroy(cavmd_recorder* r);
/* Rewrites rows first .. first + count - 1 from HOST memory after synchronising the stream of the last record call; nothing is
 * changed if a row is refused; counters and series are kept.  CAVMD_ERR_INVALID_VALUE while that stream is being captured,
 * and for a range outside the batch. */
CAVMD_API int cavmd_recorder_set_items(cavmd_recorder* r, size_t first, size_t count, const cavmd_recorder_item* h_items);
/* Enqueues exactly ONE kernel of n_items workgroups on `stream`: no allocation, no copy, no host wait.  May be captured into a
 * hipGraph, and a replay appends like an eager call: every item's call counter moves, and on every period-th call the item
 * writes row number `rows` into slot rows % capacity of its series and moves `rows`.  The kernel reads the result blocks, the
 * velocities and the net forces as they are when it RUNS and writes nothing but the series and the counters.  Workgroups
 * start in order of max(N, n_members) descending (ties in item order).  One recorder serves one stream at a time. */
CAVMD_API int cavmd_recorder_record(cavmd_recorder* r, void* stream);
/* Synchronises `stream` (the stream the record calls, or the graph that holds them, ran on), then out[i] = rows written by
 * item i since creation / the last reset.  CAVMD_ERR_INVALID_VALUE while `stream` is being captured. */
CAVMD_API int cavmd_recorder_rows(cavmd_recorder* r, void* stream, uint64_t* out);
/* Synchronises `stream`, then out[k * n_rows + j] = row first_row + j (0-based count of RECORDED rows) of item first_item + k.
 * CAVMD_ERR_NOT_COMPUTED if an item asked for has never recorded, CAVMD_ERR_INVALID_VALUE for rows at or beyond the item's
 * `rows`, n_rows or n_items 0, items outside the batch and while `stream` is being captured, CAVMD_ERR_EXPIRED if a
 * requested row has been overwritten (row < rows - capacity).  It never looks at a sequence stamp, so it works the same
 * before, between and after the replays of a graph. */
CAVMD_API int cavmd_recorder_read(cavmd_recorder* r, void* stream, size_t first_item, size_t n_items, uint64_t first_row,
                                  size_t n_rows, cavmd_record* out);
/* Zero all counters of all items (ordered on `stream`): the next recorded row is row 0, written by call 1. */
CAVMD_API int cavmd_recorder_reset(cavmd_recorder* r, void* stream);
/* Device addresses of the series (item-major: record j of item i at records[i * capacity + j % capacity]) and of the n_items
 * row counters, for consumers that stay on the GPU.  Either out pointer may be NULL. */
CAVMD_API int cavmd_recorder_device_ptr(cavmd_recorder* r, const cavmd_record** records, const uint64_t** rows);

/* ---- density field and F(k,t) of a batch, recorded on the device: the fourth kernel of the batched step ------------------ */
/* What the reference's FieldAutocorrelationTracker (src/cavitymd/analysis.py:260-418) does every step for every replica --
 * rho(k) = sum_j exp(i k . r_j) for a set of wavevectors (compute_density_field, :34-47), F_r(t) = mean_k Re(rho_r(k)
 * conj rho(k, t)) against every stored reference field (compute_field_autocorr), and now and then a new reference (act,
 * :380-414: correlate with all active references FIRST, then maybe add one) -- as ONE launch for all systems that appends one
 * 160-byte record per system to a time series kept in DEVICE memory.  Write position, reference count and the row of the last
 * reference are kept on the device too, so a hipGraph replay appends a NEW row, and takes a reference when one is due, exactly
 * like an eager call: with this a captured step is {cavmd_batch_compute, cavmd_recorder_record, cavmd_field_recorder_record,
 * cavmd_bussi_batch_step}.  The host reads when it likes, behind a synchronisation of the stream it names; nothing is mapped,
 * nothing is polled.  Systems are independent: no workgroup waits for another one, hence no CAVMD_ERR_SYNC_TIMEOUT here.
 *
 * One recording call for one item (t = rows the item has recorded so far, 0-based):
 *   1. rho(k) of the positions as they are when the kernel RUNS: the term arithmetic of cavmd_density_field
 *      (k . r = (x kx + y ky) + z kz, the same sincos and the same choice, per 64-particle tile, between the fast path and the
 *      device library's for |k . r| >= 1e8 or non-finite coordinates), plain sums in an order that depends on (N, n_k) ONLY --
 *      not on the batch, the item's place in it, the compute unit, eager or replay.  Within 1e-13 * N of the exact sum per
 *      component, within 2e-13 * N of cavmd_density_field (whose sum order differs).
 *   2. F[r] = (sum over k ascending of (a_r[k] * a[k] + b_r[k] * b[k])) / n_k for every stored reference r (a, b = Re, Im;
 *      one IEEE rounding per operation, no FMA, left to right in k from +0): bit for bit that expression on the fields
 *      cavmd_field_recorder_read_fields returns.  rho2 is the same expression with the field itself.
 *   3. The row goes to slot t % capacity.
 *   4. AFTER step 2 the field is stored as reference number n_references if fewer than max_references are stored and (none is
 *      stored yet, or reference_interval > 0 and t - (row of the last reference) >= reference_interval, or the item's word of
 *      d_take_reference is non-zero).  Row 0 therefore has n_references = 0, took_reference = 1, and the row that takes
 *      reference r does not yet contain F[r], as in the reference.
 *   5. cavmd_field_recorder_reset forgets rows, counters and references.
 * An item with N = 0 records rows of zeros and takes zero fields as references; it touches no particle array.  A call that
 * records no row (period > 1) computes nothing and ignores d_take_reference. */
#define CAVMD_FIELD_MAX_WAVEVECTORS 256
#define CAVMD_FIELD_MAX_REFERENCES 16

typedef struct cavmd_field_item          /* 64 B; DEVICE pointer */
{
    const double* d_position;            /* particle i's x, y, z at d_position + i * position_stride bytes (WRAPPED) */
    uint64_t position_stride;            /* 24 or any multiple of 8 >= 24 (32 = HOOMD's Scalar4 pos) */
    uint32_t N;                          /* 0 legal; <= CAVMD_BATCH_MAX_ITEM_N */
    uint32_t reserved0;
    uint64_t reserved[5];                /* must be 0 */
} cavmd_field_item;

typedef struct cavmd_field_record        /* 160 B, one per item and recorded call */
{
    uint64_t call;                       /* 1-based index of the record call that wrote the row */
    uint32_t n_references;               /* references the row was correlated with (F[n_references..] are 0) */
    uint32_t took_reference;             /* 1 if this call stored its field as reference number n_references */
    double rho2;                         /* mean_k |rho(k)|^2 of this call: the lag-0 value of a reference taken now */
    double reserved;                     /* 0 */
    double F[CAVMD_FIELD_MAX_REFERENCES];
} cavmd_field_record;
typedef struct cavmd_field_recorder cavmd_field_recorder; /* opaque; belongs to the workspace it was created from */

/* Per-item validation of create / set_items; host arithmetic only, needs no device.  CAVMD_ERR_INVALID_VALUE for a null item,
 * a null d_position with N > 0, a d_position not 8-byte aligned, a position_stride below 24 or not a multiple of 8,
 * reserved0 or reserved != 0; CAVMD_ERR_CAPACITY for N above CAVMD_BATCH_MAX_ITEM_N. */
CAVMD_API int cavmd_field_recorder_item_check(const cavmd_field_item* item);
/* Validates the n_items rows in HOST memory (1 .. CAVMD_BATCH_MAX_ITEMS) and copies the table and the n_k wavevectors (rows of
 * (kx, ky, kz) in HOST memory, ONE set for the whole batch: the reference builds kmag * generate_fibonacci_sphere(50) for
 * every replica, src/cavitymd/analysis.py:296-306) to the device of `ws`, once.  Allocates n_items x capacity records, n_items x
 * (max_references + 1) fields and the per-item counters in device memory, all zero.  Every `period`-th record call writes a
 * row.  reference_interval counts RECORDED ROWS; 0 = no automatic reference after the first.  CAVMD_ERR_INVALID_VALUE unless
 * 1 <= n_k <= CAVMD_FIELD_MAX_WAVEVECTORS with finite components, capacity >= 1, period >= 1 and
 * 1 <= max_references <= CAVMD_FIELD_MAX_REFERENCES; CAVMD_ERR_CAPACITY if series plus fields would exceed 1 GiB.
 * cavmd_destroy answers CAVMD_ERR_INVALID_VALUE and frees nothing while a field recorder of the workspace is alive.  Without a
 * device there is no workspace, hence no field recorder. */
CAVMD_API int cavmd_field_recorder_create(cavmd_workspace* ws, size_t n_items, const cavmd_field_item* h_items, size_t n_k,
                                          const double* h_wavevectors, size_t capacity, uint64_t period,
                                          uint32_t max_references, uint64_t reference_interval, cavmd_field_recorder** out);
/* Synchronises the stream of the last record call (unless that stream is being captured), then frees. */
CAVMD_API int cavmd_field_recorder_destroy(cavmd_field_recorder* r);
/* Rewrites rows first .. first + count - 1 from HOST memory after synchronising the stream of the last record call; nothing is
 * changed if a row is refused; counters, series and references are kept.  CAVMD_ERR_INVALID_VALUE while that stream is being
 * captured, and for a range outside the batch. */
CAVMD_API int cavmd_field_recorder_set_items(cavmd_field_recorder* r, size_t first, size_t count,
                                             const cavmd_field_item* h_items);
/* Enqueues exactly ONE kernel of n_items workgroups on `stream`: no allocation, no copy, no host wait.  May be captured into a
 * hipGraph; a replay appends like an eager call.  d_take_reference is NULL or a DEVICE array of n_items uint32_t read when the
 * kernel RUNS (like cavmd_bussi_batch_step's inputs; CAVMD_ERR_INVALID_VALUE if not 4-byte aligned): a non-zero word asks
 * that item to take a reference at this call (step 4).  That is how a caller implements the reference's time-based
 * reference_interval_ps under an adaptive timestep; the policy stays the caller's.  Workgroups start in order of N
 * descending (ties in item order).  One field recorder serves one stream at a time. */
CAVMD_API int cavmd_field_recorder_record(cavmd_field_recorder* r, void* stream, const uint32_t* d_take_reference);
/* Synchronises `stream`, then out[i] = rows written by item i since creation / the last reset.  CAVMD_ERR_INVALID_VALUE while
 * `stream` is being captured. */
CAVMD_API int cavmd_field_recorder_rows(cavmd_field_recorder* r, void* stream, uint64_t* out);
/* Synchronises `stream`, then out[k * n_rows + j] = row first_row + j (0-based count of RECORDED rows) of item first_item + k.
 * CAVMD_ERR_NOT_COMPUTED if an item asked for has never recorded, CAVMD_ERR_INVALID_VALUE for rows at or beyond the item's
 * `rows`, n_rows or n_items 0, items outside the batch and while `stream` is being captured, CAVMD_ERR_EXPIRED if a
 * requested row has been overwritten (row < rows - capacity). */
CAVMD_API int cavmd_field_recorder_read(cavmd_field_recorder* r, void* stream, size_t first_item, size_t n_items,
                                        uint64_t first_row, size_t n_rows, cavmd_field_record* out);
/* Synchronises `stream`, then for one item: rho_now = the field of its last recorded call (2 n_k doubles, h_out[2k] = Re,
 * h_out[2k+1] = Im, as cavmd_density_field_read), rho_refs = its stored reference fields one after the other (room for
 * max_references x 2 n_k doubles; *n_refs of them are written), ref_rows = the row each was taken at (room for max_references),
 * *n_refs = how many are stored.  rho_now, rho_refs and ref_rows may each be NULL.  CAVMD_ERR_NOT_COMPUTED if the item has
 * never recorded (also after a reset), CAVMD_ERR_INVALID_VALUE for an item outside the batch, a null n_refs and while `stream`
 * is being captured. */
CAVMD_API int cavmd_field_recorder_read_fields(cavmd_field_recorder* r, void* stream, size_t item, double* rho_now,
                                               double* rho_refs, uint64_t* ref_rows, uint32_t* n_refs);
/* Zero all counters of all items (ordered on `stream`): rows, calls and references are forgotten; the next recorded row is
 * row 0, written by call 1, and takes reference 0. */
CAVMD_API int cavmd_field_recorder_reset(cavmd_field_recorder* r, void* stream);
/* Device addresses of the series (item-major: record j of item i at records[i * capacity + j % capacity]) and of the n_items
 * row counters, for consumers that stay on the GPU.  Either out pointer may be NULL. */
CAVMD_API int cavmd_field_recorder_device_ptr(cavmd_field_recorder* r, const cavmd_field_record** records,
                                              const uint64_t** rows);

/* ---- the velocity-Verlet step of a batch, two launches per step: what makes the captured sequence a complete MD step ------ */
/* The reference has no integrator of its own: its driver gives the molecules to HOOMD-blue's ConstantVolume method and the one
 * cavity particle to HOOMD-blue's Langevin method (--molecular-bath bussi --cavity-bath langevin, the default of
 * examples/05_advanced_run.py:652, 677).  This section is the two half-steps of those methods for B registered systems, each
 * half ONE kernel, one 256-thread workgroup per system, all per-step inputs read from DEVICE memory when the kernel RUNS.  A
 * captured step is then {cavmd_verlet_step_one, cavmd_batch_compute, cavmd_verlet_step_two, cavmd_recorder_record,
 * cavmd_field_recorder_record, cavmd_bussi_batch_step}, and it follows an adaptive dt and fresh variates on replay.  Systems
 * are independent: no workgroup waits for another one, hence no CAVMD_ERR_SYNC_TIMEOUT here.
 *
 * The arithmetic restates TwoStepConstantVolume / TwoStepLangevin of HOOMD-blue 4.x [HOOMD upstream, not in checkout]; the
 * expressions below ARE the contract.  Every operation is one IEEE fp64 rounding, no FMA; per particle j and component c:
 *   step one   (a row with skip != 0, or an item with N == 0, leaves the item untouched)
 *     1. v_c = v_c + (0.5 * a_c) * dt
 *     2. x_c = x_c + dt * v_c
 *     3. one wrap per axis, hi = L_c * 0.5, lo = -hi: if x_c >= hi then x_c -= L_c and the image is incremented, otherwise if
 *        x_c < lo then x_c += L_c and the image is decremented
 *     4. a component still outside [lo, hi) afterwards (NaN included) is counted in out_of_box; it is not repaired
 *   step two   (the same rows are left untouched)
 *     1. minv = 1.0 / m
 *     2. F_c = ((f0_c + f1_c) + f2_c) + f3_c over the force arrays present
 *     3. d_net_force, if given, receives (F_x, F_y, F_z, the same left-to-right sum of .w)
 *     4. for j == langevin_index with langevin_gamma != 0, v being the velocity from BEFORE the kick:
 *        bd_c = uniform_c * langevin_coeff - langevin_gamma * v_c;  F_c = F_c + bd_c
 *     5. a_c = F_c * minv, stored to d_accel
 *     6. v'_c = v_c + (0.5 * a_c) * dt, stored to d_vel; then, for the particle of item 4, with v' the velocity just stored
 *        (from AFTER the kick):
 *        tally = (bd_x * v'_x + bd_y * v'_y) + bd_z * v'_z;  langevin_reservoir = langevin_reservoir - tally * dt
 *     7. steps += 1
 *   cavmd_verlet_accelerations is 1, 2, 3 and 5 only: no Langevin, no kick, nothing counted, no input row.
 * What item 4 amounts to.  `uniform` must be FRESH for every step and every item: three new variates, uniform in [-1, 1)
 * (mean 0, variance 1/3), independent of the item's velocity; variates from [0, 1), or the same three on every step, integrate
 * without any sign of trouble and heat the particle to several kT.  For a particle of mass m that feels no force but the bath,
 * with x = langevin_gamma * dt / (2 m), 0 < x < 1, the stationary state has, per component:
 *     after step two   m <v^2> = kT, for any dt        (the kick is v' = (1 - x) v + n with <n^2> = x kT / m)
 *     after step one   m <v^2> (1 - x) = kT            (the half-step velocity, the one item 4 reads)
 *     langevin_reservoir gains 0 per step on average, for every 0 < x < 1: bd acts through this kick and the next step's first
 *     kick with one acceleration, v -> v' -> v'', v + v'' = 2 v', so bd . v' dt is exactly the kinetic energy it gives, and
 *     -tally * dt what the bath took.  cavmd_ledger_row.universe_total is therefore conserved to the integrator's own error.
 *     (Taken with the velocity from BEFORE the kick, as versions of this header before the ledger's column was rehearsed had
 *     it, the tally misses the noise's heating and the reservoir grows by 3 gamma kT dt / (m (1 - x)) per step.)
 * (tests/langevin_twin.py derives the three and the reservoir's spread; tests/test_gpu_langevin_batch.py holds the kernels to
 * them; tests/thermostatted_twin.py and tests/test_gpu_conserved_energy.py hold the ledger's column to its band.)
 * pos.w (the type tag) and vel.w (the mass) are never written.  Langevin on more than one particle per system is the next
 * section's (cavmd_bath_*: the 3 N variates are drawn inside step two).  Out of scope: rotational degrees of freedom, triclinic
 * boxes. */
typedef struct cavmd_verlet_item         /* 128 B; all pointers DEVICE pointers; the arrays of one item must not overlap */
{
    cavmd_double4* d_pos;                /* HOOMD Scalar4 positions (wrapped), type tag in .w; 16-byte aligned */
    cavmd_int3* d_image;                 /* 4-byte aligned */
    cavmd_double4* d_vel;                /* HOOMD Scalar4 velocities, mass in .w; 16-byte aligned */
    double* d_accel;                     /* packed N x 3 (HOOMD's Scalar3), caller-owned, 8-byte aligned: written by
                                            cavmd_verlet_accelerations / step_two, read by step_one */
    const cavmd_double4* d_force[4];     /* summed left to right; [0] non-NULL when N > 0; the list ends at the first NULL;
                                            16-byte aligned */
    cavmd_double4* d_net_force;          /* NULL, or receives the sum (16-byte aligned) */
    double Lx, Ly, Lz;
    uint32_t N;                          /* 0 is legal: nothing of the item is read or written; <= CAVMD_BATCH_MAX_ITEM_N */
    int32_t langevin_index;              /* -1: none; else < N: the particle coupled to the Langevin bath */
    uint64_t reserved[3];                /* must be 0 */
} cavmd_verlet_item;
typedef struct cavmd_verlet_input        /* 64 B; one row per item, in DEVICE memory, owned by the caller */
{
    double dt;
    double langevin_gamma;               /* 0: no bath this step */
    double langevin_coeff;               /* sqrt(6 gamma kT / dt), taken on the host (cavmd_verlet_input_make) */
    double uniform[3];                   /* three variates uniform in [-1, 1) */
    uint64_t skip;                       /* != 0: dt == 0, the item is left untouched by both half-steps */
    uint64_t reserved;
} cavmd_verlet_input;
typedef struct cavmd_verlet_state        /* 32 B; one per item, in device memory */
{
    uint64_t steps;                      /* second half-steps applied */
    uint64_t out_of_box;                 /* coordinates left outside the box by step one (a dt or a force gone wrong) */
    double langevin_reservoir;           /* HOOMD's reservoir energy of the Langevin method: - sum of tally * dt */
    double reserved;
} cavmd_verlet_state;
typedef struct cavmd_verlet cavmd_verlet; /* opaque; belongs to the workspace it was created from */

/* Per-item validation of create / set_items; host arithmetic only, needs no device.  CAVMD_ERR_INVALID_VALUE for a null item,
 * reserved != 0, a misaligned array, a null d_pos / d_image / d_vel / d_accel / d_force[0] with N > 0, a non-NULL d_force entry
 * after a NULL one, a langevin_index below -1 or not below N; CAVMD_ERR_CAPACITY for N above CAVMD_BATCH_MAX_ITEM_N. */
CAVMD_API int cavmd_verlet_item_check(const cavmd_verlet_item* item);
/* Fills one input row on the HOST: langevin_coeff = sqrt(6 * gamma * kT / dt) (0 for gamma == 0 or dt == 0), skip = (dt == 0),
 * as c = exp(-deltaT / tau) is taken on the host for the thermostat batch.  Needs no device.  CAVMD_ERR_INVALID_VALUE for a
 * null `uniform` or `row`.  The caller copies rows to its device array. */
CAVMD_API int cavmd_verlet_input_make(double dt, double gamma, double kT, const double uniform[3], cavmd_verlet_input* row);
/* Validates the n_items rows in HOST memory (1 .. CAVMD_BATCH_MAX_ITEMS), copies the table to the device of `ws` (set-up time)
 * and allocates one zeroed state per item on the device.  cavmd_destroy answers CAVMD_ERR_INVALID_VALUE and frees nothing while
 * an integrator of the workspace is alive.  Without a device there is no workspace, hence no integrator. */
CAVMD_API int cavmd_verlet_create(cavmd_workspace* ws, size_t n_items, const cavmd_verlet_item* h_items, cavmd_verlet** out);
/* Synchronises the stream of the last launch (unless that stream is being captured), then frees. */
CAVMD_API int cavmd_verlet_destroy(cavmd_verlet* v);
/* Rewrites rows first .. first + count - 1 from HOST memory after synchronising the stream of the last launch; nothing is
 * changed if a row is refused; the items' states are kept.  CAVMD_ERR_INVALID_VALUE while that stream is being captured, and
 * for a range outside the batch. */
CAVMD_API int cavmd_verlet_set_items(cavmd_verlet* v, size_t first, size_t count, const cavmd_verlet_item* h_items);
/* Each of the three calls below enqueues exactly ONE kernel of n_items workgroups on `stream`: no allocation, no copy, no host
 * wait; may be captured into a hipGraph.  Workgroups start in order of N descending (ties in item order).  d_inputs: n_items
 * rows in DEVICE memory (CAVMD_ERR_INVALID_VALUE if null or not 8-byte aligned), read when the kernel RUNS: the caller
 * refreshes that buffer, in stream order, between replays; the pointer itself is frozen at capture.  Both half-steps of one
 * step must see the same rows.  One integrator serves one host thread and one stream at a time. */
/* a = F / m from the force arrays as they are (and the net force, if asked for): what HOOMD does once at the start of a run. */
CAVMD_API int cavmd_verlet_accelerations(cavmd_verlet* v, void* stream);
CAVMD_API int cavmd_verlet_step_one(cavmd_verlet* v, void* stream, const cavmd_verlet_input* d_inputs);
CAVMD_API int cavmd_verlet_step_two(cavmd_verlet* v, void* stream, const cavmd_verlet_input* d_inputs);
/* A kick with a force that is none of the items' d_force arrays: what the impulse multiple-time-step scheme (Verlet-I /
 * r-RESPA) needs around n plain steps -- the LONG part of a split Coulomb batch, weight n / 2 before and after them.  Enqueues
 * exactly ONE kernel of n_items 256-thread workgroups, tiles as in step two; may be captured.  d_forces: a DEVICE array of
 * n_items DEVICE pointers (N entries each, 16-byte aligned), owned by the caller; the pointers, the input rows and the items'
 * rows are all read when the kernel RUNS.  For an item with skip == 0, N > 0 and a non-NULL force pointer, per particle and
 * component, every operation one rounding, no FMA:
 *     h = weight * dt;   minv = 1.0 / m;   v_c = v_c + (f_c * minv) * h
 * and NOTHING else is written: vel.w, d_accel, d_net_force, the state and its `steps` keep their bytes.  A skipped item, an
 * item with N == 0 and an item whose pointer is NULL are left untouched.  CAVMD_ERR_INVALID_VALUE for a null handle, a null
 * or not 8-byte aligned d_inputs or d_forces, and a weight that is not finite.  The scheme is defined for a dt that is the
 * same through an outer step (the fixed mode of cavmd_draw); under the adaptive rule it is unsupported, and an end time of the
 * run clock that falls inside an outer step leaves that item with an unmatched opening kick: nothing is built for either. */
CAVMD_API int cavmd_mts_verlet_kick(cavmd_verlet* v, void* stream, const cavmd_verlet_input* d_inputs,
                                const cavmd_double4* const* d_forces, double weight);
/* Synchronises `stream`, then out = the n_items states.  CAVMD_ERR_INVALID_VALUE while `stream` is being captured. */
CAVMD_API int cavmd_verlet_read(cavmd_verlet* v, void* stream, cavmd_verlet_state* out);
/* Zero the states of all items (ordered on `stream`). */
CAVMD_API int cavmd_verlet_reset(cavmd_verlet* v, void* stream);
/* Device address of the n_items states (indexed by item), for consumers that stay on the GPU. */
CAVMD_API int cavmd_verlet_state_device_ptr(cavmd_verlet* v, const cavmd_verlet_state** out);

/* ---- a Langevin bath on any set of particles of a batch, drawn in step two: the driver's --molecular-bath langevin ------------ */
/* The reference's driver has three choices for --molecular-bath (examples/05_advanced_run.py:649-666): `bussi` is the thermostat
 * batch, `none` the integrator alone, and `langevin` HOOMD-blue's Langevin method on every molecular particle with
 * tally_reservoir_energy=True.  This section is the third: an object created from an integrator whose ONE launch takes the
 * place of cavmd_verlet_step_two in a step (it is never called in addition to it) and couples any subset of each item's
 * particles to a bath.  The 3 N variates are drawn inside the kernel from the counter-based generator of the next section
 * (Philox4x32-10, its item 1) and never touch memory; nothing new is launched.  A captured step is then {cavmd_draw_fill,
 * cavmd_verlet_step_one, the forces, cavmd_bath_step_two, cavmd_recorder_record, ...}; for --molecular-bath langevin
 * --cavity-bath langevin the cavity particle simply carries its own gamma in d_gamma.  d_net_force receives the forces WITHOUT
 * any bath term, so the adaptive dt's force_mass_sum excludes the bath, as the reference's does.  One 256-thread workgroup per
 * item, in the integrator's launch order; no workgroup waits for another, hence no CAVMD_ERR_SYNC_TIMEOUT here.
 *
 * The expressions below ARE the contract (tests/bath_mirror.py restates them); one IEEE fp64 rounding per operation, no FMA.
 * Items 1, 2, 3, 5, 6 and 7 of step two are unchanged: a row with skip != 0, or an item with N == 0, leaves the item and its
 * bath state untouched; d_net_force receives the sum of the force arrays; steps += 1.  Item 4 stays what it is for
 * j == langevin_index with langevin_gamma != 0: that particle takes the ROW's bath and not this object's.  New, for every other
 * particle j with j < the bath item's N and gamma_j > 0 (anything else, a NaN included, is not coupled and adds nothing), `draws`
 * being the item's counter in DEVICE memory when the kernel RUNS:
 *   1. Generator.  Philox4x32-10 as in the next section.  Key = (seed low, seed high) of the ITEM.  Counter = (draws low,
 *      draws high, j, 0x80000000 + b), b = 0, 1: the fourth word keeps these counters apart from cavmd_draw's purposes (all below
 *      48) even under equal keys.
 *   2. Variates, as the next section's item 2: u_x from w0,w1 and u_y from w2,w3 of block 0, u_z from w0,w1 of block 1, each
 *      2 * (k * 2^-53) - 1, in [-1, 1).
 *   3. coeff_j = sqrt(((6 * gamma_j) * kT) / dt), division and square root correctly rounded.
 *   4. bd_c = u_c * coeff_j - gamma_j * v_c with v from BEFORE the kick;  F_c = F_c + bd_c;  then the integrator's items 5
 *      and 6, and with v' the velocity item 6 stores (from AFTER the kick):
 *      tally_j = (bd_x * v'_x + bd_y * v'_y) + bd_z * v'_z
 *   5. Per item: coupled = the number of such particles; T = the sum of their tally_j, a compensated (double-double) sum in an
 *      order that depends on N only -- not on the batch, the item's place in it, the compute unit, or eager launch versus graph
 *      replay -- rounded once, within 2 ulp of the exact sum of those addends;  reservoir = reservoir - T * dt;  draws += 1.
 *      An item with d_gamma NULL has none of this done and none of its state written.
 * Two properties.  An item without a bath (d_gamma NULL, or no gamma_j > 0) gets from cavmd_bath_step_two exactly the bytes
 * cavmd_verlet_step_two gives it.  The closed forms of the Langevin paragraph above hold for every coupled free particle, with
 * its own gamma_j and mass (tests/bath_twin.py; tests/test_gpu_bath_batch.py holds the kernel to them).
 * The limits.  The variates are Philox with the counter layout published here, not HOOMD's RandomGenerator: no draw is
 * bit-comparable with a HOOMD run; everything after the draw is held to the expressions above.  Rotational degrees of freedom
 * and triclinic boxes stay out of scope. */
typedef struct cavmd_bath_item           /* 64 B; pointers are DEVICE pointers */
{
    const double* d_gamma;   /* N doubles, 8-byte aligned, caller-owned: the friction of every particle (HOOMD's per-type gamma,
                                spelled out per particle; a filter is "gamma 0 outside it").  NULL with N == 0: no bath on this item */
    uint64_t seed;           /* the Philox key of THIS item: its variates do not depend on its place in a batch */
    double kT;               /* finite, >= 0 */
    uint32_t N;              /* doubles behind d_gamma; particles at or beyond it are not coupled; <= CAVMD_BATCH_MAX_ITEM_N */
    uint32_t reserved0;      /* 0 */
    uint64_t reserved[4];    /* 0 */
} cavmd_bath_item;
typedef struct cavmd_bath_state          /* 32 B, one per item, device memory */
{
    uint64_t draws;          /* second half-steps this object applied to the item (the generator's step counter) */
    uint64_t coupled;        /* particles that received the bath in the last such step */
    double reservoir;        /* HOOMD's reservoir energy of the Langevin method, summed over the item's coupled particles */
    double reserved;
} cavmd_bath_state;
typedef struct cavmd_bath cavmd_bath;    /* opaque; belongs to the integrator it was created from */

/* Per-item validation of create / set_items; host arithmetic only, needs no device.  CAVMD_ERR_INVALID_VALUE for a null item,
 * reserved words that are not 0, a d_gamma not 8-byte aligned, d_gamma NULL with N != 0 or non-NULL with N == 0, a kT that is
 * negative or not finite; CAVMD_ERR_CAPACITY for N above CAVMD_BATCH_MAX_ITEM_N. */
CAVMD_API int cavmd_bath_item_check(const cavmd_bath_item* item);
/* Item i of the bath belongs to item i of the integrator `v`: n_items must equal the integrator's item count
 * (CAVMD_ERR_INVALID_VALUE otherwise, as for a null `v`, `h_items` or `out`).  Validates the rows in HOST memory, copies the table
 * to the integrator's device (set-up time), allocates one zeroed state per item and synchronises the device.  While a bath lives,
 * cavmd_verlet_destroy answers CAVMD_ERR_INVALID_VALUE and frees nothing: the rule cavmd_destroy has for its dependents. */
CAVMD_API int cavmd_bath_create(cavmd_verlet* v, size_t n_items, const cavmd_bath_item* h_items, cavmd_bath** out);
/* Synchronises the stream of the last cavmd_bath_step_two (unless that stream is being captured), then frees. */
CAVMD_API int cavmd_bath_destroy(cavmd_bath* b);
/* Rewrites rows first .. first + count - 1 from HOST memory after synchronising the stream of the last cavmd_bath_step_two;
 * nothing is changed if a row is refused; the items' states are kept.  CAVMD_ERR_INVALID_VALUE while that stream is being
 * captured, and for a range outside the table. */
CAVMD_API int cavmd_bath_set_items(cavmd_bath* b, size_t first, size_t count, const cavmd_bath_item* h_items);
/* Enqueues exactly ONE kernel of n_items workgroups on `stream`, in place of cavmd_verlet_step_two: the same argument checks
 * (CAVMD_ERR_INVALID_VALUE for a null or not 8-byte aligned d_inputs), the same launch order (N descending), no allocation, no
 * copy, no host wait; may be captured into a hipGraph, and a replay draws like an eager call.  The integrator notes the stream:
 * cavmd_verlet_set_items and cavmd_verlet_destroy wait for it too. */
CAVMD_API int cavmd_bath_step_two(cavmd_bath* b, void* stream, const cavmd_verlet_input* d_inputs);
/* Synchronises `stream`, then out = the n_items states.  CAVMD_ERR_INVALID_VALUE while `stream` is being captured. */
CAVMD_API int cavmd_bath_read(cavmd_bath* b, void* stream, cavmd_bath_state* out);
/* Zero the states of all items (ordered on `stream`), `draws` included: after it the same variates come again. */
CAVMD_API int cavmd_bath_reset(cavmd_bath* b, void* stream);
/* Device address of the n_items states (indexed by item), for consumers that stay on the GPU. */
CAVMD_API int cavmd_bath_state_device_ptr(cavmd_bath* b, const cavmd_bath_state** out);

/* ---- the start of a batch: seeded momenta and the photon's placement in ONE launch: the driver's thermalize_system ------------- */
/* The sections above and below cover every step of the reference driver's run; this one covers its start.  Before the first
 * step the driver thermalises the molecular momenta and draws a velocity for the cavity particle
 * (examples/05_advanced_run.py:710-750, thermalize_system), and it places the cavity particle at q = 0 or, with --finite-q, at
 * -d g / omegac^2 with the z component zeroed, adds a thermal spread sqrt(kT / omegac^2) where g != 0, wraps the position and
 * sets the image flags (:455-494, create_cavity_particle) -- all on the host, with one numpy generator walked through the
 * systems in order.  Here ONE kernel does it for all items, one 256-thread workgroup per item in the launch order the other
 * objects use (N descending, stable), reading the molecular dipole where it lives: in the item's result block of the cavity
 * batch.  It is seeded and counted like the bath: the variates of an item are a function of (its seed, its `draws`, the
 * particle, the component) alone, so a system's start does not depend on its place in a batch, and a captured launch draws a
 * new block with every replay -- re-thermalising between segments of a run needs no host work.  No workgroup waits for another,
 * hence no CAVMD_ERR_SYNC_TIMEOUT here.  The order of a start is {cavmd_batch_compute (the dipole), cavmd_thermalize_run,
 * cavmd_batch_compute and the other forces again (a moved photon makes the earlier ones stale), cavmd_verlet_accelerations}.
 *
 * The expressions below ARE the contract (tests/thermalize_mirror.py restates them); one IEEE fp64 rounding per operation, no
 * FMA; division and square root are correctly rounded.  One run of one item, `draws` being the item's counter in DEVICE memory
 * when the kernel RUNS:
 *   1. Generator.  Philox4x32-10 exactly as item 1 of "the step inputs of a batch" below, words to doubles as its item 2.  Key =
 *      (seed low, seed high) of the ITEM.  Counter = (draws low, draws high, j, purpose).  Velocity component c = 0, 1, 2 of
 *      particle j uses purpose 0xC0000000 + c; component c of the photon's position uses purpose 0xC0000008 + c, with j the
 *      photon's index.  This range is apart from cavmd_draw's purposes (all below 48) and from the bath's (0x80000000 + b) even
 *      under equal keys.  A normal n is that section's item 3, sqrt(-2 * log(u1)) * cospi(2 * u2) with u1 from w0,w1 (an
 *      argument of log) and u2 from w2,w3 of ONE block: one block per normal.
 *   2. Members.  The set is the list d_members[0 .. n_members), or with d_members NULL every j < N except the photon of item
 *      4 (every j < N when item 4 names none).  For each j of the set with j < N and a mass m = d_vel[j].w that is finite and
 *      > 0:  sigma = sqrt(kT / m);  v_c = sigma * n_c, c = 0, 1, 2.  .w keeps its bits: the row is written with one 16-byte
 *      and one 8-byte store, as the integrator writes it.  Any other j of the set (an index >= N, which is never
 *      dereferenced; a mass that is 0, negative, infinite or a NaN) leaves its row untouched and is counted in `skipped`;
 *      `thermalised` is the number of rows written.  The indices of a list must be distinct: this is NOT checked, and two
 *      entries naming one particle race.
 *   3. CAVMD_THERMALIZE_ZERO_MOMENTUM.  P_c = the sum over the thermalised j of m * v_c, each addend rounded once; a
 *      compensated (double-double) sum in an order that depends on N and the member list only -- entry k of the set belongs
 *      to lane k mod 256 (tiles of CAVMD_THERMALIZE_TILE entries walked in order, a shuffle tree over the wave, the four waves
 *      in wave order: the fold of the bath's tally), not on the batch, the item's place in it, the compute unit, or eager launch
 *      versus graph replay -- rounded once, within 2 ulp of the exact sum of those addends.  Then, for every thermalised j,
 *      v_c = v_c - (P_c / (double)thermalised) / m.  `momentum` = P; it is 0 when the flag is off or nothing was thermalised.
 *      This restates HOOMD-blue 4.x ParticleGroup::thermalizeParticleMomenta (normal velocities of variance kT / m, then the
 *      centre-of-mass momentum shared out as P / n per particle) FROM KNOWLEDGE: HOOMD is not in the checkout, and parity with
 *      it is pinned by nothing.
 *   4. The photon.  Only with d_result, and only if that block's n_particles == N and 0 <= photon_idx < N; otherwise `photon` =
 *      -1 and nothing of this item is done, which is not an error (the no-photon rule of cavmd_compute_hoomd).  With p =
 *      photon_idx, K and g = couplstr from `params`, d = the block's dipole, after every store of items 2 and 3:
 *        CAVMD_THERMALIZE_PHOTON_VELOCITY   v_c = sqrt(kT / d_vel[p].w) * n_c with j = p and the velocity purposes; no
 *                                           momentum term (the driver's :729 at mass 1); a mass that is not finite and > 0
 *                                           leaves the row untouched
 *        CAVMD_THERMALIZE_PLACE_PHOTON      x_c = FINITE_Q ? ((-d_c) * g) / K : 0 for c = 0, 1, and x_z = 0;
 *                                           if g != 0:  x_c = x_c + sqrt(kT / K) * n_c for all three c (position purposes);
 *                                           i_c = floor((x_c + L_c / 2) / L_c);  pos_c = x_c - i_c * L_c;
 *                                           d_image[p] = i as int32;  d_pos[p].w keeps its bits
 *      These are the driver's lines :464-494; at phmass = 1 (K = omegac^2) they are bit for bit the same expressions.  A list
 *      that names p thermalises it as a member first; PHOTON_VELOCITY then overwrites that row.
 *   5. Counters.  draws += 1 per run of an item, also when its set is empty; an item with N == 0 is untouched, its state
 *      included.  cavmd_thermalize_reset zeroes the states, so the same variates come again.
 * The limits.  The variates are Philox with the counter layout published here, not HOOMD's RandomGenerator and not numpy's: no
 * start is bit-comparable with a HOOMD run; log and cospi are the device library's (tests/draw_mirror.py derives the bound
 * between two implementations); everything else is held to the expressions above.  Angular momenta and triclinic boxes stay out
 * of scope. */
#define CAVMD_THERMALIZE_ZERO_MOMENTUM 1u  /* item 3 */
#define CAVMD_THERMALIZE_PLACE_PHOTON 2u   /* item 4: position and image of the photon */
#define CAVMD_THERMALIZE_FINITE_Q 4u       /* item 4: the displaced equilibrium; needs d_result */
#define CAVMD_THERMALIZE_PHOTON_VELOCITY 8u /* item 4: the photon's velocity */
#define CAVMD_THERMALIZE_TILE 512u         /* entries of a member set per tile of the kernel: T of item 3's order */
typedef struct cavmd_thermalize_item     /* 160 B; all pointers DEVICE pointers */
{
    cavmd_double4* d_vel;          /* N rows, 16-byte aligned, mass in .w; required with N != 0 */
    const uint32_t* d_members;     /* n_members indices, 4-byte aligned; NULL (with n_members 0): the default set of item 2.
                                      Not NULL with n_members 0: the empty set */
    cavmd_double4* d_pos;          /* the arrays of the cavity batch's item (16 / 4-byte aligned); required by PLACE_PHOTON */
    cavmd_int3* d_image;
    const cavmd_result* d_result;  /* this item's block of cavmd_batch_results_device_ptr, 8-byte aligned; NULL: no photon */
    uint64_t seed;                 /* the Philox key of THIS item, as cavmd_bath_item.seed */
    double kT;                     /* finite, >= 0 */
    uint32_t N;                    /* <= CAVMD_BATCH_MAX_ITEM_N */
    uint32_t n_members;            /* <= CAVMD_BATCH_MAX_ITEM_N */
    uint32_t flags;                /* CAVMD_THERMALIZE_* */
    uint32_t reserved0;            /* 0 */
    double L[3];                   /* the box edges; finite, >= 0, and > 0 with PLACE_PHOTON */
    cavmd_params params;           /* 32 B; every field finite and >= 0, K > 0 with PLACE_PHOTON */
    uint64_t reserved[4];          /* 0 */
} cavmd_thermalize_item;
typedef struct cavmd_thermalize_state    /* 64 B, one per item, device memory; only the item's workgroup writes it, plain stores */
{
    uint64_t draws;                /* runs of this item (the generator's counter) */
    uint64_t thermalised;          /* rows item 2 wrote in the last run */
    uint64_t skipped;              /* entries of the set it left untouched */
    double momentum[3];            /* P of item 3 */
    int32_t photon;                /* the photon of item 4 in the last run, -1 for none */
    uint32_t reserved0;
    uint64_t reserved;
} cavmd_thermalize_state;
typedef struct cavmd_thermalize cavmd_thermalize; /* opaque; belongs to the workspace it was created from */

/* Per-item validation of create / set_items; host arithmetic only, needs no device.  CAVMD_ERR_INVALID_VALUE for a null item,
 * reserved words that are not 0, an unknown flag, a misaligned pointer, d_vel NULL with N != 0, d_members NULL with n_members
 * != 0, a kT, box edge or params field that is negative or not finite, FINITE_Q without d_result, PLACE_PHOTON without d_pos,
 * d_image or d_result, or with a box edge or K that is 0; CAVMD_ERR_CAPACITY for N or n_members above CAVMD_BATCH_MAX_ITEM_N. */
CAVMD_API int cavmd_thermalize_item_check(const cavmd_thermalize_item* item);
/* Validates the n_items rows in HOST memory (1 .. CAVMD_BATCH_MAX_ITEMS), copies the table to the device of `ws` (set-up time)
 * and allocates one zeroed state per item on the device.  cavmd_destroy answers CAVMD_ERR_INVALID_VALUE and frees nothing while
 * a thermalize object of the workspace is alive.  Without a device there is no workspace, hence no thermalize object. */
CAVMD_API int cavmd_thermalize_create(cavmd_workspace* ws, size_t n_items, const cavmd_thermalize_item* h_items,
                                      cavmd_thermalize** out);
/* Synchronises the stream of the last launch (unless that stream is being captured), then frees. */
CAVMD_API int cavmd_thermalize_destroy(cavmd_thermalize* t);
/* Rewrites rows first .. first + count - 1 from HOST memory after synchronising the stream of the last launch; nothing is
 * changed if a row is refused; the items' states are kept.  CAVMD_ERR_INVALID_VALUE while that stream is being captured, and
 * for a range outside the table.  A launch captured earlier finds the new rows through the table. */
CAVMD_API int cavmd_thermalize_set_items(cavmd_thermalize* t, size_t first, size_t count, const cavmd_thermalize_item* h_items);
/* Enqueues exactly ONE kernel of n_items workgroups on `stream`: no allocation, no copy, no host wait; may be captured into a
 * hipGraph, and a replay draws like an eager call.  It must be ordered after the cavmd_batch_compute whose dipole it reads and
 * before every launch that reads the velocities or the photon's position.  One object serves one stream at a time. */
CAVMD_API int cavmd_thermalize_run(cavmd_thermalize* t, void* stream);
/* Synchronises `stream`, then out = the n_items states.  CAVMD_ERR_INVALID_VALUE while `stream` is being captured. */
CAVMD_API int cavmd_thermalize_read(cavmd_thermalize* t, void* stream, cavmd_thermalize_state* out);
/* Zero the states of all items (ordered on `stream`), `draws` included: after it the same variates come again. */
CAVMD_API int cavmd_thermalize_reset(cavmd_thermalize* t, void* stream);
/* Device address of the n_items states (indexed by item), for consumers that stay on the GPU. */
CAVMD_API int cavmd_thermalize_state_device_ptr(cavmd_thermalize* t, const cavmd_thermalize_state** out);

/* ---- the energy ledger of a batch: every term of the conserved energy per step, recorded on the device in ONE launch ---------- */
/* What the reference's EnergyTracker (src/cavitymd/analysis.py:425-1046) writes per output step for every replica -- the
 * potential of every force, the three cavity energies, the molecular, cavity and total kinetic energy, the system total, the
 * reservoir energy of every bath and universe_total_energy, the column it marks [CONSERVED] -- as ONE launch for all systems that
 * appends one 192-byte row per system to a time series kept in DEVICE memory.  One 256-thread workgroup per item; the write
 * position lives on the device, so a hipGraph replay appends a NEW row each time, exactly as cavmd_recorder_record does, and the
 * host reads the series when it likes.  Every pointer of an item is a DEVICE pointer that is read when the kernel RUNS: the .w
 * column of the force arrays (each particle's share of the energy), the cavmd_result block, the velocities, and single doubles
 * inside the state arrays of the objects above and below (&cavmd_bussi_device_state[i].reservoir_translational,
 * &cavmd_verlet_state[i].langevin_reservoir, &cavmd_bath_state[i].reservoir, &cavmd_draw_state[i].elapsed).  The kernel writes
 * nothing but the series and the counters; no workgroup waits for another, hence no CAVMD_ERR_SYNC_TIMEOUT here.
 *
 * The expressions in cavmd_ledger_row ARE the contract; one IEEE fp64 rounding per +, * and /, no FMA.  Per item and row:
 *   - potential[t] is the sum of d_energy[t][j].w over j < N: a fixed-order compensated (double-double) sum rounded once, in an
 *     order that depends on N only, within 2 ulp of the exact sum where sum |w| / |sum w| <= 2^40 (the bound stated for
 *     cavmd_record's sums above); an absent term is +0;
 *   - kinetic_group has the bits of cavmd_record.kinetic_energy and kinetic_cavity those of cavmd_record.cavity_kinetic, for the
 *     same velocities, member list and result block;
 *   - cavity[], reservoir[] and time are the bytes the pointers held when the kernel ran.
 * temperature is the group's: (2 * KE) / (dof * kB).  The reference's own column, (2/3) * KE / (3 * n * kB) with n molecular
 * particles (analysis.py's EnergyTracker), is this expression with dof = 9 n; the usual kinetic temperature is dof = 3 n.
 * One .w per force array: the reference's harmonic / lj and ewald_short / ewald_long columns are not split here; a caller who
 * wants them apart creates two force batches and names two terms. */
typedef struct cavmd_ledger_row          /* 192 B, one per item and recorded call */
{
    uint64_t call;            /* 1-based index of the cavmd_ledger_record call (of this item) that wrote the row */
    uint32_t n_terms;         /* the item's non-NULL d_energy entries */
    uint32_t n_reservoirs;    /* the item's non-NULL d_reservoir entries */
    double time;              /* *d_time, or 0 */
    double potential[4];      /* sum of .w per term; absent terms +0 */
    double cavity[3];         /* harmonic, coupling, dipole-self: bytes of cavmd_result.energy; 0 without d_result */
    double cavity_potential;  /* (cavity[0] + cavity[1]) + cavity[2] */
    double potential_total;   /* (((potential[0] + potential[1]) + potential[2]) + potential[3]) + cavity_potential */
    double kinetic_group;     /* kinetic energy of the item's group */
    double kinetic_cavity;    /* kinetic energy of the cavity particle (cavmd_result.photon_idx); 0 without one */
    double kinetic_total;     /* kinetic_group + kinetic_cavity if add_cavity_kinetic, else kinetic_group */
    double system_total;      /* kinetic_total + potential_total */
    double reservoir[4];      /* the bytes each pointer held; absent reservoirs +0 */
    double reservoir_total;   /* ((reservoir[0] + reservoir[1]) + reservoir[2]) + reservoir[3] */
    double universe_total;    /* system_total + reservoir_total: the reference's [CONSERVED] column */
    double temperature;       /* (2.0 * kinetic_group) / (dof * kB), or 0 where dof == 0 */
    double reserved;          /* 0 */
} cavmd_ledger_row;

typedef struct cavmd_ledger_item         /* 128 B; all pointers DEVICE pointers, read when the kernel runs */
{
    const cavmd_result* d_result;        /* the cavity force's block, e.g. cavmd_batch_results_device_ptr + item; NULL: the three
                                            cavity energies and kinetic_cavity are 0 (the driver's --no-cavity) */
    const cavmd_double4* d_vel;          /* Scalar4 velocities, mass in .w; NULL: the kinetic columns are 0 */
    const uint32_t* d_members;           /* group of kinetic_group, or NULL = 0 .. n_members-1 */
    uint32_t n_members;                  /* <= CAVMD_BATCH_MAX_ITEM_N; 0 is legal (kinetic_group 0) */
    uint32_t N;                          /* entries of every d_energy array; <= CAVMD_BATCH_MAX_ITEM_N; 0 is legal */
    const cavmd_double4* d_energy[4];    /* Scalar4 force arrays of N entries whose .w is summed; no non-NULL entry after a NULL
                                            one (cavmd_verlet_item.d_force's rule) */
    const double* d_reservoir[4];        /* each the address of ONE double, 8-byte aligned; the same NULL rule */
    const double* d_time;                /* e.g. &cavmd_draw_state[i].elapsed; NULL: time is 0 */
    double dof;                          /* finite, >= 0: the degrees of freedom behind `temperature` */
    uint32_t add_cavity_kinetic;         /* 0 or 1: 1 where the group leaves the cavity particle out */
    uint32_t reserved0;                  /* must be 0 */
    uint64_t reserved;                   /* must be 0 */
} cavmd_ledger_item;
typedef struct cavmd_ledger cavmd_ledger; /* opaque; belongs to the workspace it was created from */

/* Per-item validation of create / set_items; host arithmetic only, needs no device.  CAVMD_ERR_INVALID_VALUE for a null item,
 * reserved words that are not 0, a d_result / d_vel / d_energy[t] not 16-byte, a d_reservoir[r] / d_time not 8-byte or a
 * d_members not 4-byte aligned, a non-NULL d_energy or d_reservoir entry after a NULL one, a dof that is negative or not finite,
 * add_cavity_kinetic above 1; CAVMD_ERR_CAPACITY for N or n_members above CAVMD_BATCH_MAX_ITEM_N. */
CAVMD_API int cavmd_ledger_item_check(const cavmd_ledger_item* item);
/* As cavmd_recorder_create, with rows of 192 bytes: validates the n_items rows in HOST memory (1 .. CAVMD_BATCH_MAX_ITEMS),
 * copies the table to the device of `ws` (set-up time) and allocates n_items x capacity rows plus the per-item counters in
 * device memory, all zero.  Every `period`-th call of cavmd_ledger_record writes a row; an item keeps its last `capacity` rows.
 * capacity >= 1, period >= 1, kB > 0 and finite (Hartree/K), else CAVMD_ERR_INVALID_VALUE; CAVMD_ERR_CAPACITY if the series
 * would exceed 1 GiB.  cavmd_destroy answers CAVMD_ERR_INVALID_VALUE and frees nothing while a ledger of the workspace is
 * alive.  Without a device there is no workspace, hence no ledger. */
CAVMD_API int cavmd_ledger_create(cavmd_workspace* ws, size_t n_items, const cavmd_ledger_item* h_items, size_t capacity,
                                  uint64_t period, double kB, cavmd_ledger** out);
/* Synchronises the stream of the last cavmd_ledger_record call (unless that stream is being captured), then frees. */
CAVMD_API int cavmd_ledger_destroy(cavmd_ledger* l);
/* Rewrites rows first .. first + count - 1 from HOST memory after synchronising the stream of the last record call; nothing is
 * changed if a row is refused; counters and series are kept.  CAVMD_ERR_INVALID_VALUE while that stream is being captured,
 * and for a range outside the batch. */
CAVMD_API int cavmd_ledger_set_items(cavmd_ledger* l, size_t first, size_t count, const cavmd_ledger_item* h_items);
/* Enqueues exactly ONE kernel of n_items workgroups on `stream`: no allocation, no copy, no host wait.  May be captured into a
 * hipGraph, and a replay appends like an eager call: every item's call counter moves, and on every period-th call the item
 * writes row number `rows` into slot rows % capacity of its series and moves `rows`.  Workgroups start in order of
 * max(N, n_members) descending (ties in item order).  One ledger serves one stream at a time. */
CAVMD_API int cavmd_ledger_record(cavmd_ledger* l, void* stream);
/* Synchronises `stream`, then out[i] = rows written by item i since creation / the last reset.  CAVMD_ERR_INVALID_VALUE while
 * `stream` is being captured. */
CAVMD_API int cavmd_ledger_rows(cavmd_ledger* l, void* stream, uint64_t* out);
/* Synchronises `stream`, then out[k * n_rows + j] = row first_row + j (0-based count of RECORDED rows) of item first_item + k;
 * the statuses of cavmd_recorder_read: CAVMD_ERR_NOT_COMPUTED if an item asked for has never recorded,
 * CAVMD_ERR_INVALID_VALUE for rows at or beyond the item's `rows`, n_rows or n_items 0, items outside the batch and while
 * `stream` is being captured, CAVMD_ERR_EXPIRED if a requested row has been overwritten (row < rows - capacity). */
CAVMD_API int cavmd_ledger_read(cavmd_ledger* l, void* stream, size_t first_item, size_t n_items, uint64_t first_row,
                                size_t n_rows, cavmd_ledger_row* out);
/* Zero all counters of all items (ordered on `stream`): the next recorded row is row 0, written by call 1. */
CAVMD_API int cavmd_ledger_reset(cavmd_ledger* l, void* stream);
/* Device addresses of the series (item-major: row j of item i at series[i * capacity + j % capacity]) and of the n_items row
 * counters, for consumers that stay on the GPU.  Either out pointer may be NULL. */
CAVMD_API int cavmd_ledger_device_ptr(cavmd_ledger* l, const cavmd_ledger_row** series, const uint64_t** rows);

/* ---- the step inputs of a batch, drawn on the device: seeded variates and an adaptive dt in ONE launch per step ------------- */
/* What fills the two input tables above and below when a captured step replays: for every registered item, ONE kernel writes
 * its cavmd_verlet_input row and its cavmd_bussi_batch_input row from a counter-based, seeded generator and computes the
 * step's dt -- fixed, or the rule of the reference's AdaptiveTimestepUpdater (src/cavitymd/simulation.py:57-92) on the
 * force_mass_sum the recorder wrote last.  A captured step is then {cavmd_draw_fill, cavmd_verlet_step_one, the forces,
 * cavmd_verlet_step_two, cavmd_recorder_record, cavmd_field_recorder_record, cavmd_bussi_batch_step}: the same seed and items
 * give the same trajectory of inputs, the dt never visits the host, and the elapsed time of every item is kept next to it.
 * One LANE per item, 256-thread workgroups; no workgroup waits for another, hence no CAVMD_ERR_SYNC_TIMEOUT here.  The
 * integrator and the thermostat are not changed: rows written by their callers in other ways keep working.
 *
 * The expressions below ARE the contract (tests/draw_mirror.py restates them).  One call for one item, `draws` being the
 * item's counter in DEVICE memory when the kernel RUNS (read, then advanced by one: a graph replay draws a new block):
 *   1. Generator.  Philox4x32-10 with the published constants (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9,
 *      0xBB67AE85).  Key = (seed low, seed high).  Counter = (draws low, draws high, item index, purpose).  A block is the
 *      four output words w0 .. w3 of one counter.  The purposes, none used twice:
 *        0            w0,w1 -> uniform[0] and w2,w3 -> uniform[1] of the integrator row (the Langevin variates)
 *        1            w0,w1 -> uniform[2]
 *        2            the thermostat's normal variate (u1 from w0,w1; u2 from w2,w3)
 *        3            w0,w1 -> the boost uniform of a gamma shape below 1
 *        16 + 2 t     the normal x of gamma try t, t = 0 .. 15 (as purpose 2)
 *        17 + 2 t     w0,w1 -> the acceptance uniform u of gamma try t
 *      Known answers (counter, key -> output): 0 0 0 0, 0 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8; ffffffff x4, ffffffff x2
 *      -> 408f276d 41c83b0e a20bc7c6 6d5451fd; 243f6a88 85a308d3 13198a2e 03707344, a4093822 299f31d0 -> d16cfe09 94fdcceb
 *      5001e420 24126ea1.
 *   2. Words to doubles, exact: k = (w_hi << 21) | (w_lo >> 11) with w_hi the first word of the pair.  A uniform in [0, 1) is
 *      k * 2^-53; a Langevin variate is 2 * that - 1, in [-1, 1) as step two demands; an argument of log is (k + 1) * 2^-53,
 *      in (0, 1].
 *   3. Normal: sqrt(-2 * log(u1)) * cospi(2 * u2), u1 an argument of log, u2 a uniform in [0, 1).
 *   4. Gamma of shape a >= 1 (Marsaglia and Tsang 2000): d = a - 1/3, c = 1 / sqrt(9 d); try t: v = (1 + c x)^3 as
 *      ((1 + c x) * (1 + c x)) * (1 + c x); accepted if v > 0 and log(u) < (((0.5 x) x + d) - d v) + d log(v); the variate is
 *      d v of the first accepted try.  At most 16 tries; if all fail the variate is d and `exhausted` is incremented (the
 *      acceptance is 0.95 at a = 1 and rises with a).  Shape a < 1: the shape-(a + 1) variate times u^(1/a), taken as
 *      exp(log(u) / a), u the boost uniform as an argument of log.
 *      bussi_dof as BussiReservoirBatch.draw_inputs has it: the normal is drawn where dof != 0 (else 0), the gamma variate of
 *      shape (dof - 1) / 2 where dof > 1 (else 0).
 *   4a. End time (only once cavmd_runclock_draw_set_end was called for the object; t_end = the item's, +0: none; `elapsed` as
 *      the call finds it).  t_end > 0 and elapsed >= t_end: the item is AT REST -- both rows are the bytes
 *      cavmd_verlet_input_make / cavmd_bussi_batch_input_make give for dt = 0 with every variate +0 (skip = 1, langevin_coeff =
 *      0, c = tau != 0 ? 1 : 0), no block is consumed, draws, dt, elapsed, tolerance and exhausted are NOT written, and
 *      `finished` (cavmd_draw_state.reserved[0]) becomes 1; items 5 and 6 do not apply.  Otherwise the call is items 5 and 6
 *      and `finished` is written 0.  A NaN elapsed compares false: such an item never finishes.  The last step is not clamped:
 *      an item stops at the first elapsed >= t_end, as the reference's ElapsedTimeTracker does.
 *   5. dt.  Fixed mode (d_records NULL): dt = dt_initial; langevin_coeff and c are the bytes cavmd_verlet_input_make and
 *      cavmd_bussi_batch_input_make give for it, taken on the HOST at create / set_items; `tolerance` is 0.  Adaptive mode:
 *        tolerance = tolerance_time_constant != 0
 *                        ? tolerance_target - (tolerance_target - tolerance_initial) * exp(-elapsed / tolerance_time_constant)
 *                        : tolerance_target
 *        rows = *d_rows;  rows == 0: dt = dt_initial;  otherwise S = d_records[(rows - 1) % capacity].force_mass_sum and
 *        dt = S > 0 and finite ? min(max(sqrt(tolerance / S), dt_min), dt_max)
 *                              : the last dt this object used for the item (dt_initial if draws == 0)
 *        langevin_coeff = gamma != 0 and dt != 0 ? sqrt(((6 * gamma) * kT) / dt) : 0;   c = tau != 0 ? exp(-dt / tau) : 0
 *      `elapsed` is in the caller's time units (the conversion to ps is the caller's), and so is tolerance_time_constant.
 *      Division and square root are correctly rounded, every operation outside log / exp / cospi is one IEEE rounding, no FMA.
 *   6. skip = (dt == 0) in both rows; draws += 1; elapsed = elapsed + dt (a plain left-to-right sum); the reserved words of
 *      the rows written are 0.  A row whose destination is NULL is not written and its variates are not computed; the other
 *      row's values do not depend on that.
 *   7. A launch captured before a cavmd_draw_set_items finds the new items through the table; lanes beyond n_items leave. */
typedef struct cavmd_draw_item           /* 160 B; all pointers DEVICE pointers */
{
    cavmd_verlet_input* d_verlet_row;    /* this item's row of the integrator's table, 8-byte aligned; NULL: not written */
    cavmd_bussi_batch_input* d_bussi_row; /* this item's row of the thermostat's table, 8-byte aligned; NULL: not written;
                                            both NULL is refused */
    const cavmd_record* d_records;       /* NULL: fixed dt = dt_initial; else the item's series (cavmd_recorder_device_ptr's
                                            records + item * capacity), 8-byte aligned */
    const uint64_t* d_rows;              /* the item's row counter (cavmd_recorder_device_ptr's rows + item); required with
                                            d_records, 8-byte aligned */
    uint64_t capacity;                   /* of that series; > 0 with d_records */
    double langevin_gamma;               /* the integrator row's constants; all doubles here finite and >= 0 */
    double langevin_kT;
    double bussi_set_T;                  /* the thermostat row's constants */
    double bussi_tau;                    /* 0: c = 0 */
    double bussi_dof;                    /* item 4 */
    double dt_initial;                   /* the fixed dt; in adaptive mode the dt while nothing is recorded */
    double tolerance_target;             /* adaptive mode */
    double tolerance_initial;
    double tolerance_time_constant;      /* 0: no ramp */
    double dt_min, dt_max;               /* the clamp of the adaptive dt; dt_min <= dt_max */
    uint64_t reserved[4];                /* must be 0 */
} cavmd_draw_item;
typedef struct cavmd_draw_state          /* 64 B; one per item, in device memory; written with plain stores by the item's lane */
{
    uint64_t draws;                      /* launches that wrote this item */
    double dt;                           /* the last dt used */
    double elapsed;                      /* the left-to-right sum of every dt handed out */
    double tolerance;                    /* the last tolerance used (0 in fixed mode) */
    uint64_t exhausted;                  /* gamma draws none of whose 16 tries was accepted */
    uint64_t reserved[3];                /* [0]: `finished`, 1 while the item rests behind its end time (the run clock's
                                            section, below), else 0; [1], [2]: 0 */
} cavmd_draw_state;
typedef struct cavmd_draw cavmd_draw;    /* opaque; belongs to the workspace it was created from */

/* Per-item validation of create / set_items; host arithmetic only, needs no device.  CAVMD_ERR_INVALID_VALUE for a null item,
 * reserved != 0, a pointer not 8-byte aligned, both destinations NULL, d_records without d_rows or with capacity 0, a
 * non-finite or negative double, dt_min > dt_max. */
CAVMD_API int cavmd_draw_item_check(const cavmd_draw_item* item);
/* Validates the n_items rows in HOST memory (1 .. CAVMD_BATCH_MAX_ITEMS), takes the fixed-mode columns, copies the table to
 * the device of `ws` (set-up time) and allocates one zeroed state per item on the device.  cavmd_destroy answers
 * CAVMD_ERR_INVALID_VALUE and frees nothing while a draw object of the workspace is alive.  Without a device there is no
 * workspace, hence no draw object. */
CAVMD_API int cavmd_draw_create(cavmd_workspace* ws, uint64_t seed, size_t n_items, const cavmd_draw_item* h_items,
                                cavmd_draw** out);
/* Synchronises the stream of the last launch (unless that stream is being captured), then frees. */
CAVMD_API int cavmd_draw_destroy(cavmd_draw* d);
/* Rewrites rows first .. first + count - 1 from HOST memory after synchronising the stream of the last launch; nothing is
 * changed if a row is refused; the items' states are kept.  CAVMD_ERR_INVALID_VALUE while that stream is being captured, and
 * for a range outside the table. */
CAVMD_API int cavmd_draw_set_items(cavmd_draw* d, size_t first, size_t count, const cavmd_draw_item* h_items);
/* Enqueues exactly ONE kernel of ceil(n_items / 256) workgroups on `stream`, items in item order: no allocation, no copy, no
 * host wait; may be captured into a hipGraph, and a replay draws like an eager call.  It must be ordered before the launches
 * that read the rows and after the cavmd_recorder_record whose row it reads.  One draw object serves one stream at a time. */
CAVMD_API int cavmd_draw_fill(cavmd_draw* d, void* stream);
/* Synchronises `stream`, then out = the n_items states.  CAVMD_ERR_INVALID_VALUE while `stream` is being captured. */
CAVMD_API int cavmd_draw_read(cavmd_draw* d, void* stream, cavmd_draw_state* out);
/* Zero the states of all items (ordered on `stream`): the next launch draws block 0 again and elapsed restarts at 0. */
CAVMD_API int cavmd_draw_reset(cavmd_draw* d, void* stream);
/* Device address of the n_items states (indexed by item), for consumers that stay on the GPU. */
CAVMD_API int cavmd_draw_state_device_ptr(cavmd_draw* d, const cavmd_draw_state** out);

/* ---- harmonic bonds and Lennard-Jones pairs of a batch in ONE launch: the molecular forces of the captured step ------------ */
/* The reference's driver builds every run from the cavity force plus hoomd.md.bond.Harmonic and hoomd.md.pair.LJ(mode='shift')
 * with the neighbour list excluding bonded pairs (examples/05_advanced_run.py:556-596).  This section is those two forces for B
 * registered systems of at most CAVMD_MOLECULAR_MAX_ITEM_N particles each, in ONE kernel: a system of N particles gets
 * ceil(N / ROWS) workgroups, each stages x, y, z and the type id of its WHOLE system into LDS (28 B a particle: 56 KiB at the
 * cap, inside the 64 KiB a kernel gets without opt-in; larger systems need a cell list, which is not built here) and each of
 * its ROWS particles walks all j.  No neighbour list, no Newton's-third-law halving, no atomics, no workgroup waits for
 * another one (hence no CAVMD_ERR_SYNC_TIMEOUT), every loop is bounded by N, and EVERY entry of an item's force array is
 * written (zeros for the photon and for particles that interact with nothing: no memset pass).  The result is a further force
 * array of cavmd_verlet_item.d_force.  Electrostatics are the next section's (cavmd_coulomb_*).
 *
 * The arithmetic restates EvaluatorPairLJ, EvaluatorBondHarmonic and BoxDim::minImage of HOOMD-blue 4.x from knowledge
 * [HOOMD upstream, not in checkout]: parity with HOOMD-blue itself is NOT pinned by anything in this repository; the
 * expressions below ARE the contract.  Every operation is one IEEE fp64 rounding, no FMA; division and sqrt are correctly
 * rounded.  For particle i with stored (wrapped) coordinates x_i and type id t_i (the low 32 bits of pos.w):
 *   minimum image, per axis c:   d_c = x_i,c - x_j,c;  h = L_c * 0.5;  if (d_c >= h) d_c -= L_c; else if (d_c < -h) d_c += L_c
 *                                rsq = (d_x * d_x + d_y * d_y) + d_z * d_z
 *   bonds of i, B starting from (0, 0, 0, 0), in the order of i's partner table (the bonds that name i, in list order):
 *                                r = sqrt(rsq);  fdivr = K * (r0 / r - 1);  e = (0.5 * K) * ((r0 - r) * (r0 - r))
 *                                B_c = B_c + d_c * fdivr;  B_w = B_w + 0.5 * e
 *   pair (i, j) contributes only if j != i, j is not a bond partner of i, t_i < n_types and t_j < n_types (an out-of-range id
 *   never indexes the table) and rsq < rcutsq[t_i][t_j] (strict: rcutsq == 0 switches a type pair off); then
 *                                r2inv = 1 / rsq;  r6inv = (r2inv * r2inv) * r2inv
 *                                fdivr = (r2inv * r6inv) * ((lj1_12 * r6inv) - lj2_6)
 *                                e = r6inv * ((lj1 * r6inv) - lj2) - eshift
 *                                p_c = p_c + d_c * fdivr;  p_w = p_w + 0.5 * e          (a skipped pair adds nothing)
 *   summation order of the pair part, S = CAVMD_MOLECULAR_J_SPLIT: partial s (0 <= s < S) starts from 0 and is the left-to-
 *   right sum over j = s, s + S, s + 2 S, ...;  P = ((p_0 + p_1) + p_2) + ... + p_(S-1)
 *   F_i = B_i + P_i, component-wise, .w (the particle's share of the potential energy) included.
 * The pair constants come from cavmd_molecular_pair_make, so that the kernel and a mirror of it start from the same bits:
 *   s2 = sigma * sigma;  s6 = (s2 * s2) * s2;  lj2 = (4 * epsilon) * s6;  lj1 = lj2 * s6;  lj1_12 = 12 * lj1;  lj2_6 = 6 * lj2
 *   rcutsq = r_cut * r_cut;  eshift = 0 without shift or with r_cut == 0, else the pair energy r6inv * ((lj1 * r6inv) - lj2)
 *   at rsq = rcutsq, in the operations above. */
#define CAVMD_MOLECULAR_MAX_ITEM_N 2048 /* 28 B x 2048 = 56 KiB of LDS */
#define CAVMD_MOLECULAR_MAX_TYPES 8
#define CAVMD_MOLECULAR_MAX_BOND_TYPES 8
#define CAVMD_MOLECULAR_MAX_BONDS 4     /* bonds on one particle */
#ifndef CAVMD_MOLECULAR_J_SPLIT         /* S, one of 1, 4, 16: a compile-time constant of the library, never a run-time tunable, */
#define CAVMD_MOLECULAR_J_SPLIT 16      /* to be settled by profiles/molecular_batch/README.md; ROWS = 256 / S (cavmd_molecular_order) */
#endif
typedef struct cavmd_molecular_pair      /* 64 B; made by cavmd_molecular_pair_make */
{
    double lj1, lj2, lj1_12, lj2_6, rcutsq, eshift;
    uint64_t reserved[2];                /* must be 0 */
} cavmd_molecular_pair;
typedef struct cavmd_molecular_bond_params /* 16 B */
{
    double K, r0;
} cavmd_molecular_bond_params;
typedef struct cavmd_molecular_params    /* 4240 B */
{
    uint32_t n_types;                    /* <= 8; type ids at or above it interact with nothing */
    uint32_t n_bond_types;               /* <= 8 */
    uint64_t reserved;                   /* must be 0 */
    cavmd_molecular_pair pair[8][8];     /* symmetric: pair[a][b] and pair[b][a] hold the same bits, for a, b < n_types */
    cavmd_molecular_bond_params bond[8];
} cavmd_molecular_params;
typedef struct cavmd_molecular_bond      /* 12 B */
{
    uint32_t a, b, type;
} cavmd_molecular_bond;
typedef struct cavmd_molecular_item      /* 64 B */
{
    const cavmd_double4* d_pos;          /* DEVICE: HOOMD Scalar4 positions (wrapped), type id in .w; 16-byte aligned */
    cavmd_double4* d_force;              /* DEVICE: N entries, all written by every launch; 16-byte aligned */
    const cavmd_molecular_bond* h_bonds; /* HOST: n_bonds triples, read during create / set_items only; 4-byte aligned */
    double Lx, Ly, Lz;
    uint32_t N;                          /* 0 is legal: the item gets no workgroup; <= CAVMD_MOLECULAR_MAX_ITEM_N */
    uint32_t n_bonds;
    uint64_t reserved;                   /* must be 0 */
} cavmd_molecular_item;
typedef struct cavmd_molecular cavmd_molecular; /* opaque; belongs to the workspace it was created from */

/* The four functions below are host arithmetic and need no device. */
/* Fills one entry of the pair table as spelled out above.  CAVMD_ERR_INVALID_VALUE for a null `out` or a non-finite or
 * negative epsilon, sigma or r_cut (or a product of them that overflows). */
CAVMD_API int cavmd_molecular_pair_make(double epsilon, double sigma, double r_cut, int shift, cavmd_molecular_pair* out);
/* CAVMD_ERR_INVALID_VALUE for null, n_types or n_bond_types above 8, reserved words != 0, and among the entries in use: a
 * constant that is not finite or is negative (eshift may be negative), an asymmetric pair table. */
CAVMD_API int cavmd_molecular_params_check(const cavmd_molecular_params* params);
/* One item against the parameters it will be used with.  CAVMD_ERR_CAPACITY for N above CAVMD_MOLECULAR_MAX_ITEM_N;
 * CAVMD_ERR_INVALID_VALUE for null arguments, parameters cavmd_molecular_params_check refuses, reserved != 0, a null (with
 * N > 0) or misaligned d_pos / d_force, a null (with n_bonds > 0) or misaligned h_bonds, box lengths that are not finite and
 * positive (with N > 0), any rcutsq in use above (min(L) * 0.5)^2 (the minimum image is then not the only one), a bond index
 * not below N, a bond with a == b, a bond type not below n_bond_types, more than CAVMD_MOLECULAR_MAX_BONDS bonds on a particle. */
CAVMD_API int cavmd_molecular_item_check(const cavmd_molecular_params* params, const cavmd_molecular_item* item);
/* ROWS (particles a workgroup owns) and S (partial sums per particle) the library was compiled with; either may be NULL. */
CAVMD_API int cavmd_molecular_order(int* rows, int* j_split);
/* Validates parameters and the n_items rows in HOST memory (1 .. CAVMD_BATCH_MAX_ITEMS), builds the workgroup -> (item, first
 * particle) table (items by N descending, ties in item order; none for N == 0) and every particle's partner table from the
 * bond lists, and copies them to the device of `ws` (set-up time).  The library, not the caller, builds the partner tables: a
 * bad index is refused here and never becomes an out-of-bounds read.  The bond lists are not referenced after the call.
 * cavmd_destroy answers CAVMD_ERR_INVALID_VALUE and frees nothing while a molecular batch of the workspace is alive. */
CAVMD_API int cavmd_molecular_create(cavmd_workspace* ws, const cavmd_molecular_params* params, size_t n_items,
                                     const cavmd_molecular_item* h_items, cavmd_molecular** out);
/* Synchronises the stream of the last launch (unless that stream is being captured), then frees. */
CAVMD_API int cavmd_molecular_destroy(cavmd_molecular* m);
/* Replaces rows first .. first + count - 1 from HOST memory after synchronising the stream of the last launch; nothing is
 * changed if a row is refused.  CAVMD_ERR_INVALID_VALUE while that stream is being captured, and for a range outside the
 * batch.  A launch captured BEFORE the call keeps its number of workgroups and its LDS size (that of the largest N it was
 * captured with).  On replay it walks the NEW workgroup table (items by N descending, ties in item order, ceil(N / ROWS)
 * workgroups each) from the front as far as its captured number of workgroups reaches: the rows of the force arrays those
 * workgroups own are written -- NaN in all four components for a system larger than the captured LDS, never an out-of-bounds
 * access -- and every other entry is left as it was; workgroups beyond the new table do nothing.  The replay is right in full
 * when no item needs more workgroups or more LDS than the launch was captured with; capture again after a call that changes
 * the sizes.  A replay is not a launch the library knows of: the caller waits for replays in flight before this call. */
CAVMD_API int cavmd_molecular_set_items(cavmd_molecular* m, size_t first, size_t count, const cavmd_molecular_item* h_items);
/* Enqueues exactly ONE kernel on `stream`: no allocation, no copy, no host wait; may be captured into a hipGraph.  One batch
 * serves one host thread and one stream at a time. */
CAVMD_API int cavmd_molecular_compute(cavmd_molecular* m, void* stream);

/* ---- Ewald Coulomb forces of a batch in TWO launches: the electrostatics of the captured step ------------------------------ */
/* The reference's driver adds the pair of forces returned by make_pppm_coulomb_forces over the bond-excluding neighbour list
 * (examples/05_advanced_run.py:598-608): HOOMD-blue's PPPM.  PPPM approximates the Ewald sum on a mesh (32^3, order 6, its own
 * choice of kappa in the driver).  Systems here have at most CAVMD_COULOMB_MAX_ITEM_N particles, where the sum itself is
 * cheaper than a mesh and needs no FFT, so this section IS the Ewald sum: real space over all pairs out of LDS, reciprocal
 * space as a direct sum over the K kept k-vectors.  Parity with HOOMD-blue's PPPM is NOT pinned by anything in this
 * repository [HOOMD upstream, not in checkout]: what separates the two is PPPM's discretisation error, which nobody has
 * measured.  The expressions below ARE the contract.  Units are HOOMD's: the pair energy is q_i q_j / r.
 *
 * A system: stored (wrapped) positions x, charges q (type ids play no part; the photon takes part through its charge, 0 in the
 * driver's systems), an orthorhombic box L, V = (Lx * Ly) * Lz, kappa > 0, r_cut with r_cut^2 <= (min(L) * 0.5)^2, k_cut >= 0,
 * and an exclusion list of at most CAVMD_COULOMB_MAX_EXCLUSIONS partners per particle.
 *   real space, for j != i:      d = the minimum image of x_i - x_j by the molecular section's rule;  rsq = (d_x d_x + d_y d_y)
 *                                + d_z d_z;  r = sqrt(rsq);  g = (2 kappa / sqrt(pi)) exp(-(kappa r)^2)
 *     j not excluded and rsq < r_cut^2 (strict):   e = q_i q_j erfc(kappa r) / r;   f/r = q_i q_j (erfc(kappa r) / r + g) / rsq
 *     j an exclusion partner of i (no cut-off):    e = -q_i q_j erf(kappa r) / r;   f/r = -q_i q_j (erf(kappa r) / r - g) / rsq
 *                                (erf itself, never erfc - 1);  F_i += d * (f/r);  w_i += 0.5 * e
 *   reciprocal space:            H = the integer triples m with mx > 0, or mx == 0 and my > 0, or mx == my == 0 and mz > 0;
 *                                k_c = (2 pi * m_c) / L_c;  k2 = (kx kx + ky ky) + kz kz, kept if 0 < k2 <= k_cut * k_cut, in
 *                                the order mx, then my, then mz ascending (K of them: cavmd_coulomb_k_count)
 *                                a_k = (4 pi / V) exp(-k2 / (4 kappa^2)) / k2  (host arithmetic, the library's table)
 *                                S(k) = sum_j q_j exp(i k.x_j) = A + i B;  theta = k.x_i
 *                                F_i += 2 q_i a_k k (A sin theta - B cos theta);  w_i += q_i a_k (A cos theta + B sin theta)
 *   self and background:         Q = sum_j q_j, taken on the device;  w_i += -(kappa / sqrt(pi)) q_i^2 - pi q_i Q / (2 V kappa^2)
 * Arithmetic is NOT fixed bit for bit: the device's erfc, erf, exp and sincos do not round like any host library's.  The
 * contract is the expressions, to the rounding bound tests/coulomb_mirror.py derives.  What is fixed: no FMA contraction, no
 * atomics, and fold orders that depend on nothing but the compile-time splits below -- the same input gives the same bits on
 * every launch and on every graph replay.
 *
 * Two launches per evaluation, and no workgroup ever waits for another one (hence no CAVMD_ERR_SYNC_TIMEOUT):
 *   1. structure factors: a system gets ceil(K / KROWS) workgroups (none for K == 0); each stages x, y, z, q of its WHOLE system
 *      into LDS (32 B a particle, 64 KiB at the cap), T = 256 / KROWS lanes share a k-vector and split the walk over j, and
 *      S(k) goes to a table the library owns (16 B per k; every slot written by its owner, no memset pass).
 *   2. forces: ceil(N / ROWS) workgroups per system with the same LDS image; S = 256 / ROWS lanes share particle i and split the
 *      walk over j (real-space and exclusion terms, and Q) and the walk over k (S(k) and the library's table of k and a_k),
 *      fold left to right, and lane 0 adds the self and background terms.  EVERY entry of an item's force array is written
 *      by every evaluation; the entry of a particle with q == 0 compares equal to zero. */
#define CAVMD_COULOMB_MAX_ITEM_N 2048    /* the molecular cap; 32 B x 2048 = 64 KiB of LDS */
#define CAVMD_COULOMB_MAX_K 4096         /* kept k-vectors of one item */
#define CAVMD_COULOMB_MAX_EXCLUSIONS 4   /* exclusion partners of one particle */
#ifndef CAVMD_COULOMB_J_SPLIT            /* S, one of 1, 4, 16, 64: lanes that share a particle in launch 2; ROWS = 256 / S */
#define CAVMD_COULOMB_J_SPLIT 16
#endif
#ifndef CAVMD_COULOMB_K_SPLIT            /* T, one of 1, 4, 16, 64: lanes that share a k-vector in launch 1; KROWS = 256 / T */
#define CAVMD_COULOMB_K_SPLIT 4          /* both are compile-time constants of the library (profiles/coulomb_batch/README.md) */
#endif
typedef struct cavmd_coulomb_item        /* 96 B */
{
    const cavmd_double4* d_pos;          /* DEVICE: HOOMD Scalar4 positions (wrapped), .w ignored; 16-byte aligned */
    const double* d_charge;              /* DEVICE: N charges, read when the kernels run; 8-byte aligned */
    cavmd_double4* d_force;              /* DEVICE: N entries, all written by every evaluation; 16-byte aligned */
    const cavmd_molecular_bond* h_exclusions; /* HOST: n_exclusions pairs in the bond-list format, `type` ignored; read during
                                            create / set_items only; 4-byte aligned */
    double Lx, Ly, Lz;
    double kappa, r_cut, k_cut;
    uint32_t N;                          /* 0 is legal: the item gets no workgroup; <= CAVMD_COULOMB_MAX_ITEM_N */
    uint32_t n_exclusions;
    uint64_t reserved;                   /* must be 0 */
} cavmd_coulomb_item;
typedef struct cavmd_coulomb cavmd_coulomb; /* opaque; belongs to the workspace it was created from */

/* The four functions below are host arithmetic and need no device. */
/* CAVMD_ERR_CAPACITY for N above CAVMD_COULOMB_MAX_ITEM_N or more than CAVMD_COULOMB_MAX_K kept k-vectors;
 * CAVMD_ERR_INVALID_VALUE for a null item, reserved != 0, a null (with N > 0) or misaligned d_pos / d_charge / d_force, a null
 * (with n_exclusions > 0) or misaligned h_exclusions, an exclusion index not below N, an exclusion with a == b, more than
 * CAVMD_COULOMB_MAX_EXCLUSIONS partners on a particle, and with N > 0: box lengths that are not finite and positive, a kappa
 * that is not finite and positive, an r_cut or k_cut that is negative or not finite, r_cut^2 above (min(L) * 0.5)^2. */
CAVMD_API int cavmd_coulomb_item_check(const cavmd_coulomb_item* item);
/* K of an item cavmd_coulomb_item_check accepts (0 for N == 0); its status otherwise. */
CAVMD_API int cavmd_coulomb_k_count(const cavmd_coulomb_item* item, uint32_t* out_K);
/* kappa = sqrt(-ln accuracy) / r_cut and k_cut = 2 kappa sqrt(-ln accuracy): both truncation errors are then of the order of
 * `accuracy`.  CAVMD_ERR_INVALID_VALUE for null outputs, an r_cut that is not finite and positive, an accuracy outside (0, 1). */
CAVMD_API int cavmd_coulomb_parameters(double r_cut, double accuracy, double* kappa, double* k_cut);
/* ROWS and S of launch 2, KROWS and T of launch 1, as the library was compiled; any may be NULL. */
CAVMD_API int cavmd_coulomb_order(int* rows, int* j_split, int* k_rows, int* k_split);
/* Validates the n_items rows in HOST memory (1 .. CAVMD_BATCH_MAX_ITEMS), builds both workgroup tables (items by N descending,
 * ties in item order), every particle's partner table from the exclusion lists and every item's table of k and a_k, and copies
 * them to the device of `ws` (set-up time).  The exclusion lists are not referenced after the call.  cavmd_destroy answers
 * CAVMD_ERR_INVALID_VALUE and frees nothing while a Coulomb batch of the workspace is alive. */
CAVMD_API int cavmd_coulomb_create(cavmd_workspace* ws, size_t n_items, const cavmd_coulomb_item* h_items, cavmd_coulomb** out);
/* Synchronises the stream of the last launch (unless that stream is being captured), then frees. */
CAVMD_API int cavmd_coulomb_destroy(cavmd_coulomb* c);
/* Replaces rows first .. first + count - 1 from HOST memory after synchronising the stream of the last launch; nothing is
 * changed if a row is refused.  CAVMD_ERR_INVALID_VALUE while that stream is being captured, and for a range outside the
 * batch.  Launches captured BEFORE the call keep their numbers of workgroups and their LDS size (that of the largest N they
 * were captured with).  On replay each walks its NEW workgroup table (items by N descending, ties in item order; ceil(K / KROWS)
 * workgroups each in launch 1, ceil(N / ROWS) in launch 2) from the front as far as its captured number of workgroups reaches;
 * workgroups beyond the new table do nothing.  Launch 2 writes the rows of the force arrays its workgroups own -- NaN in all
 * four components for a system larger than the captured LDS (launch 1 gives it NaN structure factors), never an out-of-bounds
 * access -- and leaves every other entry as it was.  Launch 1 writes the S(k) slots its workgroups own; a slot it does not
 * reach keeps the 0 this call allocates the table with, so after a call that RAISES a K the forces of an item with such a
 * slot are finite and are NOT the Ewald sum: its k-sum is short, and nothing flags it.  The replay is right in full when no
 * item needs more workgroups in either launch or more LDS than the launches were captured with (a smaller N or K is fine);
 * capture again after a call that changes N or K.  A replay is not a launch the library knows of: the caller waits for
 * replays in flight before this call. */
CAVMD_API int cavmd_coulomb_set_items(cavmd_coulomb* c, size_t first, size_t count, const cavmd_coulomb_item* h_items);
/* Enqueues exactly TWO kernels on `stream`: no allocation, no copy, no host wait; may be captured into a hipGraph.  One batch
 * serves one host thread and one stream at a time. */
CAVMD_API int cavmd_coulomb_compute(cavmd_coulomb* c, void* stream);
/* Device address of the structure-factor table, for consumers that stay on the GPU, and (either may be NULL) the HOST array of
 * n_items offsets into it: item i owns K_i + 1 entries of two doubles from offset[i] on, {A, B} of its k-vectors in the order
 * above and then {Q, 0}.  Both are valid until the next cavmd_coulomb_set_items or cavmd_coulomb_destroy. */
CAVMD_API int cavmd_coulomb_structure_device_ptr(cavmd_coulomb* c, const double** out, const uint32_t** h_offsets);

/* ---- the reciprocal-space method of a Coulomb batch: the direct sum, or per-axis phase factors (opt-in) ------------------------ */
/* The k-vectors lie on a lattice, so exp(i k.x) = E_x(mx) E_y(my) E_z(mz) with E_c(m) = exp(i m phi_c): the FACTORED method takes
 * cos theta and sin theta of the section above from three sincos per particle and about one complex multiplication per
 * (particle, k), where the DIRECT method calls sincos(k.x) once per (particle, k) in either launch.  Everything else IS the
 * section above: the same kept set and order of k-vectors, the same a_k table, the same S(k) slots (launch 1 fills {A, B}, launch 2
 * stores {Q, 0}), the same real-space, exclusion, self and background terms (the same device code), two launches, no FMA, no
 * atomics, no workgroup that waits for another.  Only (cos theta, sin theta) = P(m) is obtained differently, per particle x:
 *   base angles:     phi_c = k1_c * x_c with k1_c = (2 pi * 1) / L_c, the library's own k-component for m = 1
 *   per-axis tables: E_c(0) = (1, 0);  E_c(1) = (cos phi_c, sin phi_c), ONE device sincos per particle and axis;
 *                    E_c(m) = E_c(m - 1) * E_c(1) for m = 2 .. M_c (M_c: the item's largest |m_c|);  E_c(-m) = conj E_c(m)
 *   segments:        the kept vectors of one (mx, my) are consecutive in mz and in k; from its first mz on, such a row is cut
 *                    into segments of at most SEG = CAVMD_EWALD_SEGMENT vectors.  For a segment that starts at zs:
 *                    P(mx, my, zs) = (E_x(mx) * E_y(my)) * E_z(zs);   P(mx, my, mz + 1) = P(mx, my, mz) * E_z(1)
 *   a * b            = (a.re b.re - a.im b.im, a.re b.im + a.im b.re), each operation rounded (no FMA contraction)
 * so the multiplications behind P(m) number max(mx - 1, 0) + max(|my| - 1, 0) + max(|zs| - 1, 0) + 2 + (mz - zs), at most
 * Mx + My + Mz + SEG - 2.  Fold orders, fixed by compile-time constants of the library alone (cavmd_ewald_order):
 *   launch 1: ceil(segments / SEGROWS) workgroups per system; a workgroup walks the system in tiles of CAVMD_EWALD_TILE particles
 *             whose tables it builds in LDS (TILE * (3 (M + 1) * 16 + 8) bytes, M the largest M_c of the batch), 256 / SEGROWS
 *             lanes share a segment, lane t adds q_j P for j = t, t + 256 / SEGROWS, ... and the group folds left to right;
 *   launch 2: ceil(N / ROWS) workgroups per system; the lanes of particle i take the real-space walk as in the section above,
 *             then the segments g = s, s + 256 / ROWS, ..., each in k order, and fold left to right.
 * The same input gives the same bits on every launch and every graph replay.  The results are NOT bit-comparable with the
 * direct method's: both are held to a derived rounding bound (tests/coulomb_mirror.py, tests/coulomb_factored_mirror.py). */
#define CAVMD_EWALD_RECIPROCAL_DIRECT 0   /* one sincos per (particle, k): what a new batch uses */
#define CAVMD_EWALD_RECIPROCAL_FACTORED 1 /* per-axis phase factors */
#define CAVMD_EWALD_TILE 64               /* particles whose tables launch 1 holds in LDS at a time */
#define CAVMD_EWALD_SEGMENT 8             /* SEG */
#define CAVMD_EWALD_MAX_M 20              /* largest |m_c| of an item under the factored method: 64 * (3 * 21 * 16 + 8) = 65024 bytes
                                           * of LDS in launch 1, the most a kernel gets without opt-in (M = 21 would need 68096) */
/* The tile length, SEG and CAVMD_EWALD_MAX_M, ROWS of the factored launch 2 and SEGROWS of the factored launch 1, as the library
 * was compiled (they do not depend on CAVMD_COULOMB_J_SPLIT / CAVMD_COULOMB_K_SPLIT); any may be NULL.  Needs no device. */
CAVMD_API int cavmd_ewald_order(int* tile, int* segment, int* max_m, int* rows, int* segment_rows);
/* Selects which two kernels cavmd_coulomb_compute enqueues from now on: a host-side switch that allocates nothing, copies
 * nothing and waits for nothing (the factored method's tables are built with the others, by create and set_items).
 * CAVMD_ERR_INVALID_VALUE for a null handle, an unknown method, and while the stream of the batch's last launch is being
 * captured.  A launch that WAS captured keeps the kernels it was captured with: a graph captured under one method goes on
 * computing with that method after the switch.  CAVMD_ERR_CAPACITY, and nothing is changed, for CAVMD_EWALD_RECIPROCAL_FACTORED
 * when an item's largest |m| on some axis exceeds CAVMD_EWALD_MAX_M (a long thin box can reach 4096 inside CAVMD_COULOMB_MAX_K).
 * While the factored method is selected cavmd_coulomb_set_items refuses such an item with CAVMD_ERR_CAPACITY, whole, as it
 * refuses any bad row.  A captured factored launch keeps its LDS sizes (those of the largest N and the largest M it was
 * captured with); on replay a system with a larger N or M gets NaN structure factors and NaN forces, never an out-of-bounds
 * access. */
CAVMD_API int cavmd_ewald_set_reciprocal(cavmd_coulomb* c, int method);
/* The method of the batch.  CAVMD_ERR_INVALID_VALUE for a null handle or a null output. */
CAVMD_API int cavmd_ewald_get_reciprocal(const cavmd_coulomb* c, int* method);

/* ---- the two parts of the Ewald sum: a short and a long force array, each evaluated on its own (opt-in) ------------------------ */
/* The reference treats electrostatics as two forces: `short, long = make_pppm_coulomb_forces(...)` (examples/05_advanced_run.py:601),
 * HOOMD's pair.Ewald over the bond-excluding list and HOOMD's PPPM force, and its energy file has a column for each
 * (ewald_short_energy, ewald_long_energy).  A batch that has been given LONG arrays evaluates the sum of the Ewald section in
 * the same two groups.  Every expression is that section's; only the grouping of the terms is new:
 *   SHORT  into the item's d_force: for every j != i that is NOT an exclusion partner and has rsq < r_cut^2 (strict) the
 *          real-space term.  Partial s walks j = s, s + S, ... and the partials fold left to right (S and ROWS of
 *          cavmd_coulomb_order, whichever reciprocal method is selected).  .w is that sum: no self and no background term.
 *   LONG   into the item's long array: the erf term of the at most four exclusion partners (no cut-off) in the same j
 *          partition, Q accumulated over all j on the way; then the walk over k by the batch's reciprocal method (direct, or
 *          factored in segment order) into r;  p = p + (2 q_i) r (.w: p + q_i r), and the same fold.  Lane 0 adds the self and
 *          background terms to .w, and the owner of particle 0 stores {Q, 0} behind the structure factors, as the combined
 *          evaluation does.
 * SHORT + LONG is the Ewald sum.  It is NOT bit-comparable with cavmd_coulomb_compute, whose partials hold both groups before
 * the fold; each part is held to its own derived bound (tests/coulomb_parts_mirror.py) and the sum to the sum of the two.  With
 * k_cut = 0 and no exclusions the x, y, z of SHORT compare equal to cavmd_coulomb_compute's.  No atomics, no FMA contraction,
 * no workgroup that waits for another: the same input gives the same bits on every launch and every graph replay. */
#define CAVMD_COULOMB_PART_SHORT 1u
#define CAVMD_COULOMB_PART_LONG  2u
/* Gives every item its LONG array: a HOST array of n_items DEVICE pointers (N entries each, 16-byte aligned; NULL only for an
 * item with N == 0), or all NULL to drop the split again.  Synchronises the stream of the last launch first.
 * CAVMD_ERR_INVALID_VALUE, and nothing is changed, for a null argument, n_items that is not the batch's, a misaligned pointer, a
 * pointer equal to the item's d_force, a NULL among non-NULL pointers for an item with N > 0, and while that stream is being
 * captured.  The pointer lives in a word of the item's device row that cavmd_coulomb_compute's kernels never read, so launches
 * captured before the call follow it (a captured LONG launch that finds NULL writes nothing).  cavmd_coulomb_set_items keeps
 * every item's long pointer; on a split batch it refuses a new item whose d_force is that pointer, and one with N > 0 where the
 * pointer is NULL. */
CAVMD_API int cavmd_mts_coulomb_set_long_forces(cavmd_coulomb* c, size_t n_items, cavmd_double4* const* h_long_force);
/* Enqueues the kernels of `parts` on `stream`: CAVMD_COULOMB_PART_SHORT is ONE kernel and writes the items' d_force;
 * CAVMD_COULOMB_PART_LONG is TWO (the structure factors of the selected reciprocal method, then the long kernel) and writes the
 * long arrays; both together are three.  No allocation, no copy, no host wait; may be captured.  EVERY entry of an array a part
 * owns is written by every evaluation of that part, and nothing of the other part's array.  CAVMD_ERR_INVALID_VALUE for a null
 * handle, any other value of `parts`, and for a batch without long arrays.  What cavmd_coulomb_set_items says about launches
 * captured before it holds for these: NaN in all four components of the rows a workgroup owns for a system beyond the captured
 * LDS, in the array of the part, never an out-of-bounds access.  cavmd_coulomb_compute is not changed by a split: it writes
 * the combined sum into d_force and never touches a long array. */
CAVMD_API int cavmd_mts_coulomb_compute_parts(cavmd_coulomb* c, void* stream, unsigned parts);

/* ---- trajectory frames of a batch: positions, velocities and images recorded on the device in ONE launch --------------------- */
/* What the driver's hoomd.write.GSD (examples/05_advanced_run.py:1231-1246) saves every --gsd-output-period-ps, with the initial
 * frame written first -- the positions, images and velocities of every replica -- as ONE launch for all systems that either
 * appends one frame per system to a ring of frames kept in DEVICE memory, or moves the call counters and leaves.  One
 * 256-thread workgroup per item.  Whether a frame is due is decided on the device, from words on the device (the item's
 * counters, *d_time, the take word), so a call captured into a hipGraph records on the right replays, under an adaptive dt as
 * well, and the host reads the ring when it likes.  Every pointer of an item is a DEVICE pointer that is read when the kernel
 * RUNS.  The kernel writes nothing but the target slot and the item's five counter words (rows, calls, phase, slot, last_time);
 * no atomics, and no workgroup waits for another, hence no CAVMD_ERR_SYNC_TIMEOUT here.
 *
 * The rule of one call, per item:
 *   1. calls += 1; forced = d_take_frame != NULL && d_take_frame[item] != 0 (the word is only read, as d_take_reference is).
 *   2. With time_interval == 0: phase += 1; due = phase >= period (cavmd_recorder_record's rule).
 *      With time_interval > 0: t = *d_time; due = rows == 0 || t - last_time >= time_interval: one subtraction, one comparison,
 *      so a NaN time is never due by it (the item's first call records whatever *d_time holds).  This is
 *      _should_create_new_reference of src/cavitymd/analysis.py:366-378 with the first frame written at once, as the driver's
 *      write_at_start.
 *   3. If due || forced: the frame goes to slot rows % capacity; last_time = *d_time (or 0) and phase = 0, whatever the cause of
 *      the frame; rows += 1.  Otherwise only calls and (by the step rule) phase move, and nothing else of the item is read.
 *   4. An item with N == 0 records headers with N = 0 and touches no particle array.
 *   5. cavmd_trajectory_reset zeroes the five counters; the next call under the time rule then records.
 *
 * A frame is a cavmd_trajectory_header and three sections (cavmd_trajectory_layout; every item of an object has this one
 * layout): positions, velocities, images, each packed rows of three components (x, y, z per particle), not Scalar4.  The
 * components of particles 0 .. N-1 are the stated conversions of pos.xyz, vel.xyz and image as those arrays are when the kernel
 * runs; pos.w (the type tag) and vel.w (the mass) are never copied.  The bytes from the end of the 3 N components to the next
 * 16-byte boundary of a section are written as zero; nothing else of the slot's sections is written (a slot that held a longer
 * frame keeps that frame's tail behind them). */
#define CAVMD_TRAJECTORY_F64 0 /* exact copies, 8 bytes per component */
#define CAVMD_TRAJECTORY_F32 1 /* GSD's chunk types, 4 bytes per component: (float)x, IEEE round to nearest even; subnormal
                                  results are kept, values beyond the float range become +-inf, NaN stays NaN */
#define CAVMD_TRAJECTORY_MAX_BYTES 4294967296ull /* 2^32: of one object's ring, n_items x capacity x frame_bytes */

typedef struct cavmd_trajectory_item     /* 64 B; all pointers DEVICE pointers, read when the kernel runs */
{
    const cavmd_double4* d_pos;          /* Scalar4 wrapped positions, 16-byte aligned; .w is the type tag and is never copied */
    const cavmd_int3* d_image;           /* 4-byte aligned */
    const cavmd_double4* d_vel;          /* Scalar4 velocities, mass in .w, never copied; NULL: the velocity section is +0 */
    const double* d_time;                /* one double, 8-byte aligned, e.g. &cavmd_draw_state[i].elapsed; NULL: time is 0 */
    double Lx, Ly, Lz;                   /* the box, copied into every header */
    uint32_t N;                          /* particles; 0 is legal; <= the object's max_N */
    uint32_t reserved0;                  /* must be 0 */
} cavmd_trajectory_item;

typedef struct cavmd_trajectory_header   /* 64 B, at the start of every frame */
{
    uint64_t call;            /* 1-based index of the cavmd_trajectory_record call (of this item) that wrote the frame */
    uint64_t row;             /* 0-based frame number of the item */
    double time;              /* *d_time, or 0 */
    uint32_t N;               /* particles in this frame */
    uint32_t flags;           /* bit 0: forced by the take word; bit 1: velocities present */
    double box[3];            /* Lx, Ly, Lz */
    uint64_t reserved;        /* 0 */
} cavmd_trajectory_header;

/* (a struct tag without a typedef: the function that fills it has its name, so C and C++ callers write `struct`) */
struct cavmd_trajectory_layout           /* 48 B; with e = element_bytes and pad16(x) = x rounded up to a multiple of 16 */
{
    uint64_t frame_bytes;     /* image_offset + pad16(12 max_N) */
    uint64_t position_offset; /* 64 */
    uint64_t velocity_offset; /* 64 + pad16(3 max_N e) */
    uint64_t image_offset;    /* velocity_offset + pad16(3 max_N e) */
    uint32_t max_N;
    uint32_t format;
    uint32_t element_bytes;   /* 8 for CAVMD_TRAJECTORY_F64, 4 for CAVMD_TRAJECTORY_F32 */
    uint32_t reserved;        /* 0 */
};
typedef struct cavmd_trajectory cavmd_trajectory; /* opaque; belongs to the workspace it was created from */

/* Per-item validation of create / set_items; host arithmetic only, needs no device.  CAVMD_ERR_INVALID_VALUE for a null item or
 * reserved0 != 0, a d_pos / d_vel not 16-byte, a d_image not 4-byte or a d_time not 8-byte aligned, a null d_pos or d_image
 * with N > 0, a box length that is not finite or not > 0 with N > 0; CAVMD_ERR_CAPACITY for N above CAVMD_BATCH_MAX_ITEM_N. */
CAVMD_API int cavmd_trajectory_item_check(const cavmd_trajectory_item* item);
/* The layout of a frame of up to max_N particles; host arithmetic only, needs no device.  CAVMD_ERR_INVALID_VALUE unless
 * 1 <= max_N <= CAVMD_BATCH_MAX_ITEM_N, format is CAVMD_TRAJECTORY_F64 or CAVMD_TRAJECTORY_F32 and out is not NULL. */
CAVMD_API int cavmd_trajectory_layout(uint32_t max_N, uint32_t format, struct cavmd_trajectory_layout* out);
/* As cavmd_ledger_create, with frames of cavmd_trajectory_layout(max_N, format).frame_bytes: validates the n_items rows in HOST
 * memory (1 .. CAVMD_BATCH_MAX_ITEMS; CAVMD_ERR_CAPACITY also for an item with N > max_N), copies the table to the device of
 * `ws` (set-up time) and allocates n_items x capacity frames plus the per-item counters in device memory, all zero.
 * CAVMD_ERR_INVALID_VALUE for capacity == 0 or period == 0, a time_interval that is negative or not finite, time_interval > 0
 * with period != 1 or with an item whose d_time is NULL, and what cavmd_trajectory_layout refuses; CAVMD_ERR_CAPACITY if
 * n_items x capacity x frame_bytes exceeds CAVMD_TRAJECTORY_MAX_BYTES.  cavmd_destroy answers CAVMD_ERR_INVALID_VALUE and frees
 * nothing while a trajectory object of the workspace is alive.  Without a device there is no workspace, hence no object. */
CAVMD_API int cavmd_trajectory_create(cavmd_workspace* ws, size_t n_items, const cavmd_trajectory_item* h_items, uint32_t max_N,
                                      uint32_t format, size_t capacity, uint64_t period, double time_interval,
                                      cavmd_trajectory** out);
/* Synchronises the stream of the last cavmd_trajectory_record call (unless that stream is being captured), then frees. */
CAVMD_API int cavmd_trajectory_destroy(cavmd_trajectory* t);
/* Rewrites rows first .. first + count - 1 from HOST memory after synchronising the stream of the last record call; nothing is
 * changed if a row is refused (CAVMD_ERR_CAPACITY for N > max_N, CAVMD_ERR_INVALID_VALUE for a NULL d_time under a
 * time_interval > 0); counters and ring are kept.  CAVMD_ERR_INVALID_VALUE while that stream is being captured, and for a range
 * outside the batch. */
CAVMD_API int cavmd_trajectory_set_items(cavmd_trajectory* t, size_t first, size_t count, const cavmd_trajectory_item* h_items);
/* Enqueues exactly ONE kernel of n_items workgroups on `stream`: no allocation, no copy, no host wait.  May be captured into a
 * hipGraph, and a replay decides like an eager call, by the rule above.  d_take_frame is NULL or a DEVICE array of n_items
 * uint32_t (4-byte aligned) read when the kernel runs.  Workgroups start in order of N descending (ties in item order).  One
 * object serves one stream at a time. */
CAVMD_API int cavmd_trajectory_record(cavmd_trajectory* t, void* stream, const uint32_t* d_take_frame);
/* Synchronises `stream`, then out[i] = frames written by item i since creation / the last reset.  CAVMD_ERR_INVALID_VALUE while
 * `stream` is being captured. */
CAVMD_API int cavmd_trajectory_rows(cavmd_trajectory* t, void* stream, uint64_t* out);
/* Synchronises `stream`, then fills out[(k * n_rows + j) * frame_bytes ...] with the whole frame first_row + j (0-based count
 * of RECORDED frames) of item first_item + k; the statuses of cavmd_ledger_read: CAVMD_ERR_NOT_COMPUTED if an item asked for
 * has never recorded, CAVMD_ERR_INVALID_VALUE for frames at or beyond the item's `rows`, n_rows or n_items 0, items outside the
 * batch and while `stream` is being captured, CAVMD_ERR_EXPIRED if a requested frame has been overwritten. */
CAVMD_API int cavmd_trajectory_read(cavmd_trajectory* t, void* stream, size_t first_item, size_t n_items, uint64_t first_row,
                                    size_t n_rows, void* out);
/* Zero the five counters of all items (ordered on `stream`): the next recorded frame is row 0, written by call 1. */
CAVMD_API int cavmd_trajectory_reset(cavmd_trajectory* t, void* stream);
/* Device addresses of the ring (item-major: frame j of item i at series + (i * capacity + j % capacity) * frame_bytes) and of
 * the n_items row counters, for consumers that stay on the GPU (either may be NULL, not both). */
CAVMD_API int cavmd_trajectory_device_ptr(cavmd_trajectory* t, const void** series, const uint64_t** rows);

/* ---- the run clock: a batch run to an end time, energy and F(k,t) rows by each item's own clock ------------------------------- */
/* Under an adaptive dt every item keeps its own clock on the device (cavmd_draw_state.elapsed), and the host cannot know on
 * which replay an item reaches a given time without reading B clocks back.  The trajectory already obeys that clock (its rule
 * 2); this section does the same for the end of the run (the reference's ElapsedTimeTracker, src/cavitymd/analysis.py:1230-
 * 1259) and for the energy ledger's rows (EnergyTracker's --energy-output-period-ps and --max-energy-output-time,
 * analysis.py:692-701) and for the field recorder's rows and references (--fkt-output-period-ps and --fkt-ref-interval, the
 * reference's "PREFERRED for adaptive mode" rule, analysis.py:366-378).  A production run is then "capture once, replay until cavmd_runclock_draw_finished counts every item".
 *
 * End times (cavmd_draw).  Item 4a of the draw contract above.  An item at rest hands out skip = 1 rows, under which both
 * half-steps, the bath step and the thermostat leave the item and its states untouched (cavmd_verlet_input.skip,
 * cavmd_bussi_batch_input.skip); counters that count calls may move.  Raising an item's t_end lets it go on from where it
 * stopped: `draws` did not move while it rested, so the continued run is bit for bit the run that had the larger t_end from
 * the start.  `finished` is part of the 64-byte state: cavmd_draw_read, cavmd_draw_reset (which zeroes it) and the snapshot
 * carry it.  End times are configuration, as items are: a rebuilt object is given them again before a snapshot is loaded.
 *
 * The ledger's time rule.  The trajectory's rule 2 with t = *item.d_time when the kernel runs, thread 0 alone reading and
 * writing the item's words:
 *     due = rows == 0 || t - last_time >= time_interval;   max_time > 0 && t > max_time: not due
 * and a written row sets last_time = t.  The comparisons are IEEE: a NaN t is never due by them (as under the trajectory's
 * rule, an item's first row is written whatever *d_time holds, and a NaN last_time then lets no further row be due).  A call that is not due moves `calls` alone.  last_time is one more word per item
 * beside the four counters (whose layout is unchanged): cavmd_ledger_reset zeroes it, and while a rule is on it is a part of
 * the snapshot blob -- the blob's header then carries word0 = 1, so that a blob taken under a rule and an object without one
 * (or the reverse) meet as a header mismatch (CAVMD_ERR_INVALID_VALUE); without a rule blob and header are what they were.
 * An item at rest stops writing rows by itself, its clock standing still.
 *
 * The field recorder's time rule.  cavmd_field_item holds no clock, so the rule takes a base DEVICE pointer and a byte stride:
 * t = the double at d_time0 + item * stride_bytes when the kernel runs.  Rows are due as the ledger's, without max_time
 * (due = rows == 0 || t - last_time >= time_interval; a written row sets last_time = t; a NaN t is never due by the
 * comparison); a call whose row is not due moves `calls` alone and computes nothing, as a call inside a period does.  The
 * record's `reserved` double holds t (it stays +0 without the rule), so that lag times can be formed from what is stored.
 * With reference_time_interval > 0 the row-count condition of the reference rule (t_row - last_reference_row >=
 * reference_interval) is replaced by t - last_reference_time >= reference_time_interval; last_reference_time follows EVERY
 * reference taken, whatever its cause (the first row's, one asked for through d_take_reference, one by either interval);
 * max_references, "the first row takes one", "correlate first, then maybe add" and d_take_reference stay as they are, and
 * with reference_time_interval == 0 the row-count rule stays.  last_time and last_reference_time are two more arrays of
 * n_items doubles beside the six counters: cavmd_field_recorder_reset zeroes them, and while a rule is on they are a sixth
 * section of the snapshot blob, whose header then carries word[1] = max_references | 0x10000 -- a header mismatch against an
 * object without the rule, and the reverse.  Unlike the ledger's, this rule's values (both intervals, d_time0, the stride) are
 * NOT launch arguments: the kernel has no scalar registers to spare, so they live in device memory in front of the two time
 * arrays and are read when the kernel runs -- a captured launch of the timed kernel sees the values of a later
 * cavmd_runclock_field_set_rule.  WHICH kernel a launch is stays frozen at capture, as below.
 *
 * Captured launches.  Which kernel a call launches and the ledger's scalar rule values (time_interval, max_time) are launch arguments,
 * frozen when a launch is captured: set the rules BEFORE the capture.  A graph captured before the first cavmd_runclock_* call
 * of an object keeps the old behaviour.  The end times live in a device array whose address does not change after the first
 * cavmd_runclock_draw_set_end, so a captured launch sees later changes of the VALUES: that is how t_end is extended between
 * replays.
 *
 * Every call below synchronises the stream of the object's last launch first, as set_items does, and answers
 * CAVMD_ERR_INVALID_VALUE while that stream is being captured, for a null handle or argument, and for a value that is negative
 * or not finite. */
/* Sets the end times of items first .. first + count - 1 from HOST memory (+0: none) and writes 0 to `finished` of those items:
 * whether one of them rests is decided again by the next cavmd_draw_fill, and until then it does not count as finished.
 * CAVMD_ERR_INVALID_VALUE also for a range outside the table.  The first call makes cavmd_draw_fill launch the kernel that
 * reads end times.  The flags are written first: if the runtime then fails the copy of the end times, end times stay as they
 * were and the next cavmd_draw_fill sets the flags again by them. */
CAVMD_API int cavmd_runclock_draw_set_end(cavmd_draw* d, size_t first, size_t count, const double* h_t_end);
/* Synchronises the stream of the last cavmd_draw_fill and `stream`, then *n_finished = the items whose `finished` is not 0 (one
 * strided copy of n_items words).  CAVMD_ERR_INVALID_VALUE while either stream is being captured. */
CAVMD_API int cavmd_runclock_draw_finished(cavmd_draw* d, void* stream, uint64_t* n_finished);
/* Switches the ledger's time rule on (time_interval > 0) or off (time_interval == 0, and then max_time must be 0);
 * max_time == 0: no last time.  CAVMD_ERR_INVALID_VALUE also unless the object was created with period == 1 and every item has
 * a d_time; while the rule is on, cavmd_ledger_set_items refuses an item without d_time.  last_time is 0 until a row is written
 * under the rule; switching the rule off and on again keeps it. */
CAVMD_API int cavmd_runclock_ledger_set_rule(cavmd_ledger* l, double time_interval, double max_time);
/* Switches the field recorder's time rule on (time_interval > 0) or off (time_interval == 0, and then reference_time_interval
 * must be 0).  Item i's clock is the double at d_time0 + i * stride_bytes in DEVICE memory, read when the kernel runs (in
 * practice &cavmd_draw_state[0].elapsed with stride 64).  CAVMD_ERR_INVALID_VALUE also for a rule on with a d_time0 that is NULL
 * or not 8-byte aligned, a stride below 8 or not a multiple of 8, or an object created with period != 1.  Both time words are
 * 0 until written under the rule; switching the rule off and on again keeps them. */
CAVMD_API int cavmd_runclock_field_set_rule(cavmd_field_recorder* r, const double* d_time0, uint64_t stride_bytes,
                                            double time_interval, double reference_time_interval);

/* ---- measurement hooks (bench.py's roofline leg) ---------------------------------------------- */
/* When enabled, every cavmd_compute_* brackets each of its kernels with hipEvents on `stream`. */
CAVMD_API int cavmd_profile_enable(cavmd_workspace* ws, int on);
/* Synchronises and returns the accumulated device time per kernel since the last reset:
 * ms[0] = dipole partial-sum kernel, ms[1] = finalize kernel (0 in the default two-launch mode, where the
 * finalize is the prologue of the force map), ms[2] = force-map kernel;
 * *launches = evaluations accumulated.  Resets the accumulators. */
CAVMD_API int cavmd_profile_read(cavmd_workspace* ws, double ms[3], uint64_t* launches);

/* Per-evaluation samples behind cavmd_profile_read: copies up to `cap` triples {reduce, finalize, map} in
 * milliseconds (oldest first) into out[3 * cap] and stores the count in *n.  Call BEFORE cavmd_profile_read, which
 * clears them.  At most the last 4096 evaluations are kept. */
CAVMD_API int cavmd_profile_samples(cavmd_workspace* ws, double* out, size_t cap, size_t* n);

/* ---- save and restore: what the objects of a batch run hold on the device, written out and put back, same bits -------------- */
/* A run of the captured step can be stopped between two replays and taken up in another process: every state that launches
 * write can be copied to HOST memory as one blob per object and copied back into an object of the same shape.  Nine objects
 * hold such state: cavmd_verlet, cavmd_bath, cavmd_draw, cavmd_thermalize and cavmd_bussi_batch one state per item;
 * cavmd_recorder, cavmd_ledger and cavmd_trajectory the counter words and the ring; cavmd_field_recorder those and the stored
 * fields and references.  Each has three calls, cavmd_snapshot_<object>_bytes / _save / _load, which add no kernel and launch
 * none: a synchronise and copies.
 *
 * A blob is a cavmd_snapshot_header followed by the object's device arrays VERBATIM, in this order, each section padded with
 * zero bytes to a multiple of 16:
 *   verlet, bath, draw, thermalize, bussi_batch   the n_items states (cavmd_*_state as cavmd_*_read gives them; for the
 *                                                 thermostat batch cavmd_bussi_device_state)
 *   recorder, ledger, trajectory                  the n_counters x n_items counter words (n_counters arrays of n_items, rows
 *                                                 written first), then the WHOLE ring of n_items x capacity x record_bytes
 *                                                 bytes, item-major by slot; slots never written are the zeros of creation
 *   ledger under the run clock's time rule        those two, then last_time (n_items doubles); the header's word[0] is 1
 *                                                 (0 without a rule, and the blob is then the two sections alone)
 *   field_recorder                                those two, then the row of every reference (n_items x max_references words),
 *                                                 the field of the last recorded call (n_items x n_k x 2 doubles) and the
 *                                                 references (n_items x max_references x n_k x 2 doubles)
 *   field_recorder under the run clock's time rule those five, then last_time and last_reference_time (2 x n_items doubles);
 *                                                 the header's word[1] is max_references | 0x10000
 * Because the arrays are copied as they are, after a load every read, rows and read_fields answers what it answered when the
 * blob was saved, by the rules it always had, and the next launch continues from there bit for bit.
 *
 * bytes  depends on the object's shape alone (the header's words); no synchronise, no device access.
 * save   synchronises `stream` (CAVMD_ERR_INVALID_VALUE while it is being captured, as cavmd_*_read), then writes header and
 *        sections to h_out.  `bytes` must be what cavmd_snapshot_<object>_bytes gives.  Nothing of the object changes.
 * load   CAVMD_ERR_INVALID_VALUE while `stream` is being captured and for a blob cavmd_snapshot_check refuses against the
 *        object's own shape, both before anything is touched; then waits for the object's launches in flight as
 *        cavmd_*_set_items does (CAVMD_ERR_INVALID_VALUE while that stream is being captured) and for `stream`, copies host to
 *        device and returns with the copy complete.  A refused load leaves the object as it was; a copy the runtime fails
 *        half-way leaves the sections already written.  Device addresses do not change: a graph captured before a load
 *        replays on the loaded state, and cavmd_*_device_ptr consumers stay valid.  For the thermostat batch the refusals
 *        counted in the loaded states count as reported (the next cavmd_bussi_batch_read does not answer
 *        CAVMD_ERR_BAD_PARAMS for them), cavmd_bussi_batch_read answers the loaded states also before the first step, and
 *        the host's sequence keeps counting from where it is.
 * A null object, a null buffer or a null `bytes` is CAVMD_ERR_INVALID_VALUE.
 *
 * NOT in a snapshot, and the caller's to recreate with the same arguments before a load: the item tables (every device
 * pointer of an item is of the new process), seeds given per item (cavmd_bath_item, cavmd_thermalize_item), periods,
 * intervals, kB, wavevectors and every other parameter of create, and the run clock's end times and rules (cavmd_runclock_*).
 * The draw object's seed is in the header, so a blob of
 * another seed is refused.  cavmd_batch, cavmd_shared_cavity, cavmd_molecular and cavmd_coulomb keep nothing between launches
 * that a later evaluation reads, so they have no snapshot. Result-history sequence numbers and cavmd_record.eval_sequence restart in a new process
 * (they are diagnostic).  Host-side generators that made input rows are the caller's.  The arrays the items point to
 * (positions, images, velocities, accelerations, input rows) are the caller's memory: save and restore them next to the blobs;
 * the accelerations cannot be recomputed after a step with a bath, they contain its random force. */
#define CAVMD_SNAPSHOT_MAGIC 0x3150414E53564143ull /* "CAVSNAP1" read as a little-endian word */
#define CAVMD_SNAPSHOT_VERSION 1u
#define CAVMD_SNAPSHOT_VERLET 1u
#define CAVMD_SNAPSHOT_BATH 2u
#define CAVMD_SNAPSHOT_DRAW 3u
#define CAVMD_SNAPSHOT_THERMALIZE 4u
#define CAVMD_SNAPSHOT_BUSSI_BATCH 5u
#define CAVMD_SNAPSHOT_RECORDER 6u
#define CAVMD_SNAPSHOT_LEDGER 7u
#define CAVMD_SNAPSHOT_TRAJECTORY 8u
#define CAVMD_SNAPSHOT_FIELD_RECORDER 9u

typedef struct cavmd_snapshot_header     /* 64 B at the start of every blob; every field native-endian */
{
    uint64_t magic;           /* CAVMD_SNAPSHOT_MAGIC */
    uint32_t version;         /* CAVMD_SNAPSHOT_VERSION */
    uint32_t kind;            /* CAVMD_SNAPSHOT_*: the object the blob was saved from */
    uint32_t n_items;
    uint32_t n_counters;      /* counter words per item of a series object; 0 for a state object */
    uint64_t capacity;        /* rows per item of a series object; 0 for a state object */
    uint64_t record_bytes;    /* bytes of one record (for the trajectory: of one frame); for a state object of one state */
    uint32_t word[2];         /* field_recorder: n_k, max_references; trajectory: max_N, format; draw: the seed's low and high
                                 half; 0, 0 otherwise */
    uint64_t bytes;           /* of the whole blob, this header included */
    uint32_t reserved[2];     /* must be 0 */
} cavmd_snapshot_header;

/* Host arithmetic only, needs no device: CAVMD_OK if the `bytes` bytes at `blob` begin with a header that load would accept
 * for an object whose cavmd_snapshot_<object>_bytes / _save header is *expected; CAVMD_ERR_INVALID_VALUE for a null pointer,
 * bytes shorter than the header or different from the header's `bytes`, a wrong magic, version or kind, any shape word
 * (n_items, n_counters, capacity, record_bytes, word[0], word[1], bytes) that differs from *expected, and reserved words that
 * are not 0.  Reads the first 64 bytes of the blob only; the blob need not be aligned. */
CAVMD_API int cavmd_snapshot_check(const void* blob, size_t bytes, const cavmd_snapshot_header* expected);
CAVMD_API int cavmd_snapshot_verlet_bytes(cavmd_verlet* v, size_t* bytes);
CAVMD_API int cavmd_snapshot_verlet_save(cavmd_verlet* v, void* stream, void* h_out, size_t bytes);
CAVMD_API int cavmd_snapshot_verlet_load(cavmd_verlet* v, void* stream, const void* h_in, size_t bytes);
CAVMD_API int cavmd_snapshot_bath_bytes(cavmd_bath* b, size_t* bytes);
CAVMD_API int cavmd_snapshot_bath_save(cavmd_bath* b, void* stream, void* h_out, size_t bytes);
CAVMD_API int cavmd_snapshot_bath_load(cavmd_bath* b, void* stream, const void* h_in, size_t bytes);
CAVMD_API int cavmd_snapshot_draw_bytes(cavmd_draw* d, size_t* bytes);
CAVMD_API int cavmd_snapshot_draw_save(cavmd_draw* d, void* stream, void* h_out, size_t bytes);
CAVMD_API int cavmd_snapshot_draw_load(cavmd_draw* d, void* stream, const void* h_in, size_t bytes);
CAVMD_API int cavmd_snapshot_thermalize_bytes(cavmd_thermalize* t, size_t* bytes);
CAVMD_API int cavmd_snapshot_thermalize_save(cavmd_thermalize* t, void* stream, void* h_out, size_t bytes);
CAVMD_API int cavmd_snapshot_thermalize_load(cavmd_thermalize* t, void* stream, const void* h_in, size_t bytes);
CAVMD_API int cavmd_snapshot_bussi_batch_bytes(cavmd_bussi_batch* b, size_t* bytes);
CAVMD_API int cavmd_snapshot_bussi_batch_save(cavmd_bussi_batch* b, void* stream, void* h_out, size_t bytes);
CAVMD_API int cavmd_snapshot_bussi_batch_load(cavmd_bussi_batch* b, void* stream, const void* h_in, size_t bytes);
CAVMD_API int cavmd_snapshot_recorder_bytes(cavmd_recorder* r, size_t* bytes);
CAVMD_API int cavmd_snapshot_recorder_save(cavmd_recorder* r, void* stream, void* h_out, size_t bytes);
CAVMD_API int cavmd_snapshot_recorder_load(cavmd_recorder* r, void* stream, const void* h_in, size_t bytes);
CAVMD_API int cavmd_snapshot_ledger_bytes(cavmd_ledger* l, size_t* bytes);
CAVMD_API int cavmd_snapshot_ledger_save(cavmd_ledger* l, void* stream, void* h_out, size_t bytes);
CAVMD_API int cavmd_snapshot_ledger_load(cavmd_ledger* l, void* stream, const void* h_in, size_t bytes);
CAVMD_API int cavmd_snapshot_trajectory_bytes(cavmd_trajectory* t, size_t* bytes);
CAVMD_API int cavmd_snapshot_trajectory_save(cavmd_trajectory* t, void* stream, void* h_out, size_t bytes);
CAVMD_API int cavmd_snapshot_trajectory_load(cavmd_trajectory* t, void* stream, const void* h_in, size_t bytes);
CAVMD_API int cavmd_snapshot_field_recorder_bytes(cavmd_field_recorder* r, size_t* bytes);
CAVMD_API int cavmd_snapshot_field_recorder_save(cavmd_field_recorder* r, void* stream, void* h_out, size_t bytes);
CAVMD_API int cavmd_snapshot_field_recorder_load(cavmd_field_recorder* r, void* stream, const void* h_in, size_t bytes);

/* ---- tuning / introspection ------------------------------------------------------------------- */
/* Launch knobs (for A/B measurements; the defaults are the measured best on MI355X).  name is one of
 *   "reduce_blocks_per_cu" 1..16   grid of the reduction = min(tiles, CUs * value); also the number of partials
 *   "map_blocks_per_cu"    1..16   grid of the force map
 *   "map_nt_store"         -1..2   force stores: -1 auto by N, 0 plain, 1 non-temporal, 2 write-through (sc1; measured slower
 *                                  at every size, profiles/r02/ab_store_policy.txt)
 *   "reduce_nt_load"       -1..2   -1 auto by N, 0 plain, 1 pos+image non-temporal, 2 all non-temporal
 *   "fused_finalize"       0/1     1: two launches per evaluation (finalize folded into the force map), 0: three
 *   "map_reverse"          -1..1   -1 auto by N, 1: the force map walks its tiles last-to-first, 0: first-to-last
 *   "small_system_max_n"   0..2^20 at or below this N (default 1024) one single-block launch does the whole evaluation (0 = never)
 *   "reduce_unroll"        -1,1,2  particles per lane and tile of the reduction (-1 auto by N)
 *   "persistent"           -1..1   ONE launch per evaluation (reduction, in-launch all-reduce of the partials, force map from
 *                                  charges kept in LDS): 1 whenever the grid is <= 256 blocks, 0 never (two launches),
 *                                  -1 auto: while a block's charges take at most half a CU's LDS (N <~ 2.4e6), so that two
 *                                  concurrent grids (other streams, other processes on the same GPU) can both be resident.
 *                                  The kernel's workgroups wait for each other inside the launch, which needs them all
 *                                  resident together.  TWO such grids fit side by side (registers: two 4-wave blocks per CU
 *                                  at 2 particles per lane; LDS: the auto rule); when more grids, or foreign kernels,
 *                                  hold the CUs, part of a grid cannot start.  Every wait is bounded (~0.4 s): workgroups
 *                                  that give up poison their share of the forces with NaN and LEAVE, which lets the rest
 *                                  of the grid start; the last workgroup to give up finds every partial in place and
 *                                  completes the whole evaluation alone (same fold, same bits, ~1 ms).  Such an
 *                                  evaluation is late but valid and is not reported as an error.  If it cannot be
 *                                  completed (not observed outside fault injection) the forces stay NaN and the result
 *                                  read or the NEXT cavmd_compute_* call, whichever comes first, returns
 *                                  CAVMD_ERR_SYNC_TIMEOUT (that call enqueues nothing).  After a starved evaluation the
 *                                  workspace SUSPENDS the single launch ("sync_timeout_seen" reads 1): two launches for
 *                                  2^16 evaluations, then one probe -- whoever held the CUs may have gone; a probe that
 *                                  starves again (late but valid, as before) makes the pause 8 times longer, up to 2^31;
 *                                  a pause starts over at 2^16 once the single launch has run healthy for longer than
 *                                  the last pause.  After a FAILED evaluation it stays suspended until the caller
 *                                  writes this tunable again.  A GPU known to be shared by three or more processes that
 *                                  each evaluate N > 1024 can skip the slow steps with the environment variable
 *                                  CAVMD_PERSISTENT=0, read by cavmd_create (=1 forces the single launch).
 *   "persistent_suspended" (read only)  0: no; 1: paused after a starved evaluation; 2: off after a failed one
 *   "sync_timeout_seen"    0..2    read: 1 after a starved evaluation.  Write: fault-injection hook, raises the flag of
 *                                  the host-visible block as a starved kernel would -- 1: failed, 2: completed by its last
 *                                  workgroup (the next call acts on it); write 0: forget it.
 *   "debug_spin_limit", "debug_late_block", "debug_late_ticks", "debug_suspend_first"
 *                                  test hooks of the single-launch kernel: poll rounds of its bounded waits (0 = default),
 *                                  a workgroup (index, -1 = none) that starts late by that many ticks of the 100 MHz
 *                                  clock, as if its CU had been held by another grid -- a real starved evaluation on
 *                                  demand -- and the length of the next pause in evaluations
 *   "rho_lane_particle"    -1..3   density-field mapping: 0 lane = wavevector, 1 / 2 / 3 lane = particle with 25 / 10 / 5
 *                                  wavevectors per chunk, -1 auto by n_k
 *   "rho_last_mapping"     (read only)  the mapping the last cavmd_density_field call used, 0..3, after the automatic rule;
 *                                  -1 before the first call
 *   "rho_last_blocks"      (read only)  the x extent of the grid that call launched, which is also the number of partial
 *                                  blocks its fold summed; -1 before the first call
 *   "persistent_lds_kb"    0..156  LDS budget per block of the single-launch kernel in KiB (0 = default); the charges of tiles
 *                                  beyond it are read a second time
 *   "result_history"       2..16384 slots of the result ring read by cavmd_result_at (default 64, 256 B each).  Setting it
 *                                  synchronises the workspace's last stream and reallocates the ring: the last evaluation's
 *                                  block is carried over (the synchronous getters still return it), every earlier sequence
 *                                  expires.  CAVMD_ERR_INVALID_VALUE while that stream is being captured.
 *   "persistent_balanced"  -1..1   partition of the particles over the blocks of the single-launch kernel: 0 tiles dealt
 *                                  round-robin (the two-launch path's partition: then also its bits), 1 contiguous equal
 *                                  shares, -1 auto
 * Returns CAVMD_ERR_INVALID_VALUE for an unknown name or an out-of-range value.  None of them changes results
 * beyond the last bit of the dipole (different but fixed summation trees). */
CAVMD_API int cavmd_set_tunable(cavmd_workspace* ws, const char* name, int value);
CAVMD_API int cavmd_get_tunable(cavmd_workspace* ws, const char* name, int* value);
CAVMD_API int cavmd_device_info(cavmd_workspace* ws, int* device, int* compute_units, char* arch_name, size_t arch_name_len);
CAVMD_API const char* cavmd_error_string(int status);
CAVMD_API int cavmd_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CAVMD_H_ */
