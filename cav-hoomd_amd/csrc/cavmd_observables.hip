// cavmd_observables.hip -- the observables of include/cavmd.h that work on a workspace (rows f2-f4: density field, cavity mode,
// sum |F| / m, kinetic energy, velocity rescale) and the Bussi reservoir thermostat, scalar and on the device
// (cavmd_observable_kernels.hpp).  The one unit besides cavmd_capi.hip that sees inside cavmd_workspace.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <utility>

#include "cavmd.h"
#include "cavmd_observable_kernels.hpp"
#include "cavmd_cavity_mode_kernel.hpp"
#include "cavmd_workspace.hpp"

using namespace cavmd;

namespace
{
constexpr int kScaleBlocksPerCu = 4; // velocity rescale: 256-thread blocks per CU (4 particles per lane and tile)
constexpr size_t kTicketBytes = 128;

// Scratch of the scalar reductions (sum |F| / m, kinetic energy): partials + the host-visible scalar + the ticket counter.
int ensure_scalar_scratch(cavmd_workspace* ws)
{
    if (ws->d_fm_part.ptr)
        return CAVMD_OK;
    DeviceArray<double> part;
    MappedBlock<HostScalar> host;
    DeviceArray<unsigned> ticket;
    CAVMD_HIP_TRY(part.alloc(2 * (size_t)ws->max_parts + 1));
    CAVMD_HIP_TRY(host.alloc());
    CAVMD_HIP_TRY(ticket.alloc_zeroed(kTicketBytes / sizeof(unsigned)));
    ws->d_fm_part = std::move(part);
    ws->h_fm = std::move(host);
    ws->d_fm_ticket = std::move(ticket);
    return CAVMD_OK;
}

// Wait for the scalar the fold kernel publishes: about a PCIe write after the kernel has it, instead of a copy plus a stream
// synchronisation.
int wait_scalar(cavmd_workspace* ws, hipStream_t stream, double* out)
{
    const StampWait w = wait_for_stamp(&ws->h_fm.host->ready, ws->fm_sequence, stream);
    if (w.error != hipSuccess)
        return (int)w.error;
    if (!w.arrived)
    {
        // the kernel never published (failed or aborted launch): its blocks may have left the ticket counter
        // part-way, after which no block would ever be "last" again -- put it back before reporting
        (void)hipMemsetAsync(ws->d_fm_ticket.ptr, 0, kTicketBytes, stream);
        return (int)hipErrorLaunchFailure;
    }
    *out = ws->h_fm.host->value;
    return CAVMD_OK;
}
} // namespace

extern "C"
{

int cavmd_set_wavevectors(cavmd_workspace* ws, size_t n_k, const double* h_wavevectors)
{
    if (!ws || !h_wavevectors || n_k == 0 || n_k > (size_t)1 << 20)
        return CAVMD_ERR_INVALID_VALUE;
    DeviceGuard guard(ws->device);
    // the old set goes first (its memory may be what the new one needs); from here to the commit the workspace has none
    ws->d_kvec.free();
    ws->d_rho_part.free();
    ws->d_rho.free();
    ws->h_rho.free();
    ws->rho_computed = false;
    ws->n_k = 0;
    const unsigned n_chunks = (unsigned)((n_k + kWave - 1) / kWave);
    const unsigned rho_blocks = (unsigned)ws->num_cu * 4; // capacity of the partial buffer: three 256-thread blocks per CU (lane =
                                                          // particle mapping) or one 1024-thread block per CU (lane = wavevector)
    DeviceArray<double> kvec, rho_part, rho;
    PinnedBlock<double> h_rho;
    CAVMD_HIP_TRY(kvec.alloc(3 * n_k));
    CAVMD_HIP_TRY(rho_part.alloc(2 * kWave * (size_t)n_chunks * rho_blocks));
    CAVMD_HIP_TRY(rho.alloc(2 * n_k));
    CAVMD_HIP_TRY(h_rho.alloc(2 * n_k));
    CAVMD_HIP_TRY(hipMemcpy(kvec.ptr, h_wavevectors, sizeof(double) * 3 * n_k, hipMemcpyHostToDevice));
    ws->d_kvec = std::move(kvec);
    ws->d_rho_part = std::move(rho_part);
    ws->d_rho = std::move(rho);
    ws->h_rho = std::move(h_rho);
    ws->n_k = n_k;
    ws->n_chunks = n_chunks;
    ws->rho_blocks = rho_blocks;
    return CAVMD_OK;
}

int cavmd_density_field(cavmd_workspace* ws, void* stream_, size_t N, const double* d_position, size_t position_stride)
{
    if (!ws || !d_position || position_stride < 24 || (position_stride & 7) || ((uintptr_t)d_position & 7))
        return CAVMD_ERR_INVALID_VALUE;
    if (ws->n_k == 0)
        return CAVMD_ERR_NOT_COMPUTED; // no wavevectors stored yet
    if (N > (size_t)INT_MAX)
        return CAVMD_ERR_CAPACITY;
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(ws->device);
    constexpr int kBlock = 1024;
    const size_t tiles = (N + kWave - 1) / kWave;
    unsigned gb;
    // lane = wavevector costs ceil(n_k / 64) * 64 lane-slots per particle, lane = particle n_k slots that measured 1.33x
    // as expensive each (N = 1e6: n_k = 17: 53 vs 87 us, 50: 99 vs 95, 64: 118 vs 88, 100: 170 vs 165)
    int lp = ws->rho_lane_particle;
    if (lp < 0)
        lp = (ws->n_k * 4 < (size_t)ws->n_chunks * kWave * 3) ? 3 : 0;
    if (lp)
    {
        // lane = particle: 256-thread blocks, KC wavevectors per chunk (2 KC running sums per lane in registers)
        constexpr int kLpBlock = 256;
        size_t g = (tiles + (kLpBlock / kWave) - 1) / (kLpBlock / kWave);
        if (g > ws->rho_blocks)
            g = ws->rho_blocks;
        gb = (unsigned)(g ? g : 1);
        with_constant(IntList<25, 10, 5> {}, lp == 1 ? 25 : lp == 2 ? 10 : 5, [&](auto kc) {
            constexpr int KC = decltype(kc)::value; // wavevectors per chunk
            hipLaunchKernelGGL((density_partials_lp_kernel<kLpBlock, KC>), dim3(gb, (unsigned)((ws->n_k + KC - 1) / KC)),
                               dim3(kLpBlock), 0, stream, reinterpret_cast<const char*>(d_position), position_stride, (unsigned)N,
                               ws->d_kvec.ptr, (unsigned)ws->n_k, make_sincos_coef(), ws->d_rho_part.ptr);
        });
    }
    else
    {
        size_t g = (tiles + (kBlock / kWave) - 1) / (kBlock / kWave);
        if (g > (size_t)ws->num_cu)
            g = (size_t)ws->num_cu;
        gb = (unsigned)(g ? g : 1);
        hipLaunchKernelGGL((density_partials_kernel<kBlock>), dim3(gb, ws->n_chunks), dim3(kBlock), 0, stream,
                           reinterpret_cast<const char*>(d_position), position_stride, (unsigned)N, ws->d_kvec.ptr,
                           (unsigned)ws->n_k, make_sincos_coef(), ws->d_rho_part.ptr);
    }
    CAVMD_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((density_fold_kernel<kBlock>), dim3(ws->n_chunks), dim3(kBlock), 0, stream, ws->d_rho_part.ptr,
                       gb, (unsigned)ws->n_k, ws->d_rho.ptr);
    CAVMD_HIP_TRY(hipGetLastError());
    ws->rho_stream = stream;
    ws->rho_computed = true;
    ws->rho_last_mapping = lp;
    ws->rho_last_blocks = (int)gb;
    return CAVMD_OK;
}

int cavmd_density_field_read(cavmd_workspace* ws, double* h_out)
{
    if (!ws || !h_out)
        return CAVMD_ERR_INVALID_VALUE;
    if (!ws->rho_computed)
        return CAVMD_ERR_NOT_COMPUTED;
    DeviceGuard guard(ws->device);
    CAVMD_HIP_TRY(hipMemcpyAsync(ws->h_rho.host, ws->d_rho.ptr, sizeof(double) * 2 * ws->n_k, hipMemcpyDeviceToHost, ws->rho_stream));
    CAVMD_HIP_TRY(hipStreamSynchronize(ws->rho_stream));
    memcpy(h_out, ws->h_rho.host, sizeof(double) * 2 * ws->n_k);
    return CAVMD_OK;
}

int cavmd_cavity_mode(cavmd_workspace* ws, void* stream_, const cavmd_double4* d_vel, double kB, double out[4])
{
    if (!ws || !d_vel || !out || !(kB > 0.0) || ((uintptr_t)d_vel & 15))
        return CAVMD_ERR_INVALID_VALUE;
    if (!ws->computed)
        return CAVMD_ERR_NOT_COMPUTED;
    // the photon index and E_h are read from the last evaluation's device-side result: if that evaluation was starved and
    // could not be completed, the block on the device still belongs to the evaluation BEFORE it -> say so instead
    if (consume_sync_timeout(ws) == kSyncFailed)
        return CAVMD_ERR_SYNC_TIMEOUT;
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(ws->device);
    if (!ws->d_mode.ptr)
    {
        DeviceArray<double> mode;
        MappedBlock<HostMode> host;
        CAVMD_HIP_TRY(mode.alloc(4));
        CAVMD_HIP_TRY(host.alloc());
        ws->d_mode = std::move(mode);
        ws->h_mode = std::move(host);
    }
    const cavmd_result* res = ws->d_result.ptr;
    ws->mode_sequence += 1;
    hipLaunchKernelGGL(cavity_mode_kernel, dim3(1), dim3(1), 0, stream, res, d_vel, kB, ws->d_mode.ptr, ws->h_mode.dev,
                       ws->mode_sequence);
    CAVMD_HIP_TRY(hipGetLastError());
    const StampWait w = wait_for_stamp(&ws->h_mode.host->ready, ws->mode_sequence, stream);
    if (w.error != hipSuccess)
        return (int)w.error;
    if (!w.arrived)
        return (int)hipErrorLaunchFailure;
    for (int k = 0; k < 4; ++k)
        out[k] = ws->h_mode.host->v[k];
    return CAVMD_OK;
}

int cavmd_force_mass_sum(cavmd_workspace* ws, void* stream_, size_t N, const cavmd_double4* d_net_force,
                         const cavmd_double4* d_vel, double* out)
{
    if (!ws || !d_net_force || !d_vel || !out || ((uintptr_t)d_net_force & 15) || ((uintptr_t)d_vel & 15))
        return CAVMD_ERR_INVALID_VALUE;
    if (N > (size_t)INT_MAX)
        return CAVMD_ERR_CAPACITY;
    if (N == 0)
    {
        *out = 0.0;
        return CAVMD_OK;
    }
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(ws->device);
    {
        const int st0 = ensure_scalar_scratch(ws);
        if (st0 != CAVMD_OK)
            return st0;
    }
    constexpr int kBlock = kObservableBlock, kUnroll = kObservableUnroll;
    // one block per CU: every block draws a ticket from ONE counter (~12 ns each, serialised at the memory side); with four
    // blocks per CU the 1024 tickets alone took 12 us
    const unsigned g = grid_for(N, kBlock * kUnroll, ws->num_cu, 1);
    double* d_out = ws->d_fm_part.ptr + 2 * (size_t)ws->max_parts;
    ws->fm_sequence += 1;
    hipLaunchKernelGGL((force_mass_fused_kernel<kBlock, kUnroll>), dim3(g), dim3(kBlock), 0, stream,
                       reinterpret_cast<const v2d*>(d_net_force), reinterpret_cast<const v2d*>(d_vel), (unsigned)N,
                       ws->d_fm_part.ptr, ws->d_fm_ticket.ptr, d_out, ws->h_fm.dev, ws->fm_sequence);
    CAVMD_HIP_TRY(hipGetLastError());
    return wait_scalar(ws, stream, out);
}

int cavmd_kinetic_energy(cavmd_workspace* ws, void* stream_, const cavmd_double4* d_vel, const uint32_t* d_members,
                         size_t n_members, double* out)
{
    if (!ws || !d_vel || !out || ((uintptr_t)d_vel & 15) || ((uintptr_t)d_members & 3))
        return CAVMD_ERR_INVALID_VALUE;
    if (n_members > (size_t)INT_MAX)
        return CAVMD_ERR_CAPACITY;
    if (n_members == 0)
    {
        *out = 0.0;
        return CAVMD_OK;
    }
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(ws->device);
    {
        const int st0 = ensure_scalar_scratch(ws);
        if (st0 != CAVMD_OK)
            return st0;
    }
    constexpr int kBlock = kObservableBlock, kUnroll = kObservableUnroll;
    const unsigned g = grid_for(n_members, kBlock * kUnroll, ws->num_cu, 1); // one ticket per CU, see cavmd_force_mass_sum
    double* d_out = ws->d_fm_part.ptr + 2 * (size_t)ws->max_parts;
    ws->fm_sequence += 1;
    hipLaunchKernelGGL((kinetic_fused_kernel<kBlock, kUnroll>), dim3(g), dim3(kBlock), 0, stream,
                       reinterpret_cast<const v2d*>(d_vel), d_members, (unsigned)n_members, ws->d_fm_part.ptr,
                       ws->d_fm_ticket.ptr, d_out, ws->h_fm.dev, ws->fm_sequence);
    CAVMD_HIP_TRY(hipGetLastError());
    return wait_scalar(ws, stream, out);
}

int cavmd_scale_velocities(cavmd_workspace* ws, void* stream_, cavmd_double4* d_vel, const uint32_t* d_members,
                           size_t n_members, double alpha)
{
    if (!ws || !d_vel || ((uintptr_t)d_vel & 15) || ((uintptr_t)d_members & 3))
        return CAVMD_ERR_INVALID_VALUE;
    if (n_members > (size_t)INT_MAX)
        return CAVMD_ERR_CAPACITY;
    if (n_members == 0)
        return CAVMD_OK;
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(ws->device);
    constexpr int kBlock = kObservableBlock, kUnroll = kObservableUnroll;
    const unsigned g = grid_for(n_members, kBlock * kUnroll, ws->num_cu, kScaleBlocksPerCu);
    hipLaunchKernelGGL((scale_velocities_kernel<kBlock, kUnroll>), dim3(g), dim3(kBlock), 0, stream, reinterpret_cast<v2d*>(d_vel),
                       d_members, (unsigned)n_members, alpha);
    return hip_status(hipGetLastError());
}

// ---- Bussi reservoir thermostat: the scalar rule (host arithmetic; the file is built with -ffp-contract=off) ---------
int cavmd_bussi_rescale_factor(double K, double degrees_of_freedom, double deltaT, double set_T, double tau,
                               double normal_variate, double gamma_variate, double* alpha)
{
    if (!alpha)
        return CAVMD_ERR_INVALID_VALUE;
    // src/BussiReservoirThermostat.h:186-190  c = exp(-dt / tau), 0 for tau == 0 (instantaneous thermalisation); the rest of
    // the rule (:183-213) is bussi_alpha_from_c, the function the on-device step runs too
    const double c = (tau != 0.0) ? exp(-deltaT / tau) : 0.0;
    *alpha = bussi_alpha_from_c(K, degrees_of_freedom, c, set_T, normal_variate, gamma_variate);
    return CAVMD_OK;
}

int cavmd_bussi_step(cavmd_bussi_reservoir* state, double K_translational, double dof_translational, double K_rotational,
                     double dof_rotational, double deltaT, double set_T, double tau, const double variates[4],
                     double factors[2])
{
    if (!state || !variates || !factors)
        return CAVMD_ERR_INVALID_VALUE;
    // src/BussiReservoirThermostat.h:45-48
    if (deltaT == 0.0)
    {
        factors[0] = factors[1] = 1.0;
        return CAVMD_OK;
    }
    // :57-61 "Bussi thermostat requires non-zero initial momenta."
    if ((dof_translational != 0 && K_translational == 0) || (dof_rotational != 0 && K_rotational == 0))
        return CAVMD_ERR_BAD_PARAMS;
    double at = 1.0, ar = 1.0;
    (void)cavmd_bussi_rescale_factor(K_translational, dof_translational, deltaT, set_T, tau, variates[0], variates[1], &at);
    (void)cavmd_bussi_rescale_factor(K_rotational, dof_rotational, deltaT, set_T, tau, variates[2], variates[3], &ar);
    // :86-95  energy handed to the reservoir = KE_old - KE_new = KE_old (1 - alpha^2)
    const double delta_t = K_translational * (1.0 - at * at);
    const double delta_r = K_rotational * (1.0 - ar * ar);
    state->reservoir_translational += delta_t;
    state->reservoir_rotational += delta_r;
    state->instantaneous_translational = delta_t;
    state->instantaneous_rotational = delta_r;
    factors[0] = at;
    factors[1] = ar;
    return CAVMD_OK;
}

namespace
{
int ensure_bussi_state(cavmd_workspace* ws)
{
    if (ws->d_bussi.ptr)
        return CAVMD_OK;
    DeviceArray<BussiDevice> state;
    MappedBlock<HostBussi> host;
    CAVMD_HIP_TRY(state.alloc_zeroed(1));
    CAVMD_HIP_TRY(host.alloc());
    ws->d_bussi = std::move(state);
    ws->h_bussi = std::move(host);
    return CAVMD_OK;
}
} // namespace

int cavmd_bussi_step_device(cavmd_workspace* ws, void* stream_, cavmd_double4* d_vel, const uint32_t* d_members,
                            size_t n_members, double dof_translational, double deltaT, double set_T, double tau,
                            double normal_variate, double gamma_variate)
{
    if (!ws || !d_vel || ((uintptr_t)d_vel & 15) || ((uintptr_t)d_members & 3))
        return CAVMD_ERR_INVALID_VALUE;
    if (n_members > (size_t)INT_MAX)
        return CAVMD_ERR_CAPACITY;
    hipStream_t stream = (hipStream_t)stream_;
    // The variates, c, set_T and dof travel by value in BussiStepArgs: a captured step would apply the same R and gamma on
    // every replay (a thermostat that is no longer stochastic).  Refused before anything is allocated, enqueued or counted.
    // A capture query that fails refuses too.
    if (capture_state(stream) != Capture::none)
        return CAVMD_ERR_INVALID_VALUE;
    if (deltaT == 0.0 || n_members == 0) // src/BussiReservoirThermostat.h:45-48: factors {1, 1}, counters untouched
        return CAVMD_OK;
    DeviceGuard guard(ws->device);
    {
        int st0 = ensure_scalar_scratch(ws);
        if (st0 == CAVMD_OK)
            st0 = ensure_bussi_state(ws);
        if (st0 != CAVMD_OK)
            return st0;
    }
    constexpr int kBlock = kObservableBlock, kUnroll = kObservableUnroll;
    BussiStepArgs a;
    a.dof = dof_translational;
    a.c = (tau != 0.0) ? exp(-deltaT / tau) : 0.0; // :186-190
    a.set_T = set_T;
    a.normal_variate = normal_variate;
    a.gamma_variate = gamma_variate;
    const unsigned g = grid_for(n_members, kBlock * kUnroll, ws->num_cu, 1);
    ws->bussi_sequence += 1;
    ws->bussi_stream = stream;
    hipLaunchKernelGGL((kinetic_partials_kernel<kBlock, kUnroll>), dim3(g), dim3(kBlock), 0, stream,
                       reinterpret_cast<const v2d*>(d_vel), d_members, (unsigned)n_members, ws->d_fm_part.ptr);
    CAVMD_HIP_TRY(hipGetLastError());
    const unsigned g2 = grid_for(n_members, kBlock * kUnroll, ws->num_cu, kScaleBlocksPerCu);
    hipLaunchKernelGGL((bussi_rescale_fused_kernel<kBlock, kUnroll>), dim3(g2), dim3(kBlock), 0, stream,
                       reinterpret_cast<v2d*>(d_vel), d_members, (unsigned)n_members, ws->d_fm_part.ptr, g, a, ws->d_bussi.ptr,
                       ws->h_bussi.dev, ws->bussi_sequence);
    return hip_status(hipGetLastError());
}

int cavmd_bussi_device_read(cavmd_workspace* ws, cavmd_bussi_device_state* out)
{
    if (!ws || !out)
        return CAVMD_ERR_INVALID_VALUE;
    memset(out, 0, sizeof(*out));
    if (!ws->d_bussi.ptr || ws->bussi_sequence == 0)
        return CAVMD_OK;
    DeviceGuard guard(ws->device);
    // (on the stream the last step went to, whatever stream the caller is on now)
    const StampWait w = wait_for_stamp(&ws->h_bussi.host->ready, ws->bussi_sequence, ws->bussi_stream);
    if (w.error != hipSuccess)
        return (int)w.error;
    if (!w.arrived)
        return (int)hipErrorLaunchFailure; // a launch that never published
    const BussiDevice s = ws->h_bussi.host->state;
    out->reservoir_translational = s.reservoir;
    out->instantaneous_translational = s.instantaneous;
    out->last_alpha = s.alpha;
    out->last_kinetic_energy = s.kinetic;
    out->steps = s.steps;
    out->refused = s.errors;
    if (s.errors != ws->bussi_refused_seen)
    {
        ws->bussi_refused_seen = s.errors;
        return CAVMD_ERR_BAD_PARAMS; // "Bussi thermostat requires non-zero initial momenta."
    }
    return CAVMD_OK;
}

int cavmd_bussi_device_reset(cavmd_workspace* ws, void* stream_)
{
    if (!ws)
        return CAVMD_ERR_INVALID_VALUE;
    if (!ws->d_bussi.ptr)
        return CAVMD_OK;
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(ws->device);
    // wait for the last step's publication first so that the host copy can be reset consistently
    cavmd_bussi_device_state unused;
    const int st = cavmd_bussi_device_read(ws, &unused);
    if (st != CAVMD_OK && st != CAVMD_ERR_BAD_PARAMS)
        return st;
    CAVMD_HIP_TRY(hipMemsetAsync(ws->d_bussi.ptr, 0, sizeof(BussiDevice), stream));
    memset(&ws->h_bussi.host->state, 0, sizeof(BussiDevice));
    ws->bussi_refused_seen = 0;
    return CAVMD_OK;
}

} // extern "C"
