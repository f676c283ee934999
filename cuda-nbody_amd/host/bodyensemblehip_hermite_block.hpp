// bodyensemblehip_hermite_block.hpp -- BodyEnsembleHIPHermiteBlockOrder<T, Order>: B independent systems of N bodies on the device, each
// stepped by the Hermite scheme with block time steps, all of them in the launches of one call: at 4th order nb_hermite_block_ensemble_*
// (include/nbody_hip_hermite_block_ensemble.h, libnbody_hip_hermite_block_ensemble.so), at 6th order nb_hermite6_block_ensemble_*
// (include/nbody_hip_hermite6_block_ensemble.h, libnbody_hip_hermite6_block_ensemble.so); BodyEnsembleHIPHermiteBlock<T> and
// BodyEnsembleHIPHermite6Block<T> name the two.  The state (positions, velocities, accelerations, jerks, at 6th order snaps and crackles,
// ticks, levels; system s holds bodies [s*N, (s+1)*N)), one status record per system, the summary record, the workspace and a
// synchronised snapshot are DeviceArrays (a device without room throws DeviceBadAlloc).  A refused call throws std::runtime_error
// carrying the nb_error_string name.
#pragma once

#include "device_array.hpp"
#include "hermite_calls.hpp"

#include <concepts>
#include <cstddef>
#include <cstdint>
#include <span>
#include <vector>

template <std::floating_point T, int Order> class BodyEnsembleHIPHermiteBlockOrder {
    using Calls = HermiteBlockEnsembleCalls<T, Order>;

 public:
    BodyEnsembleHIPHermiteBlockOrder(std::size_t num_bodies, std::size_t num_systems, T softening_sq, const nb_hermite_block_params_t& params)
        : num_bodies_(num_bodies), num_systems_(num_systems), softening_sq_(softening_sq), params_(params) {
        // the sizes the step refuses are refused here, before anything is allocated
        const bool fits = num_bodies <= 0xFFFFFFFFu && num_systems <= 0xFFFFFFFFu;
        hip_check(fits ? Calls::workspace_bytes.fn(n(), b(), sizeof(T), &workspace_bytes_) : NB_ERR_INVALID_ARGUMENT, Calls::workspace_bytes.name);
        const auto bodies = num_bodies * num_systems;
        pos_  = DeviceArray<T>(4 * bodies);
        vel_  = DeviceArray<T>(4 * bodies);
        acc_  = DeviceArray<T>(4 * bodies);
        jerk_ = DeviceArray<T>(4 * bodies);
        if constexpr (Order == 6) {
            snap_    = DeviceArray<T>(4 * bodies);
            crackle_ = DeviceArray<T>(4 * bodies);
        }
        pos_out_   = DeviceArray<T>(4 * bodies);
        vel_out_   = DeviceArray<T>(4 * bodies);
        ticks_     = DeviceArray<std::uint64_t>(bodies);
        levels_    = DeviceArray<std::int32_t>(bodies);
        status_    = DeviceArray<nb_hermite_block_status_t>(num_systems);
        summary_   = DeviceArray<nb_hermite_block_ensemble_summary_t>(1);
        workspace_ = DeviceArray<unsigned char>(workspace_bytes_);
    }

    auto num_bodies() const noexcept { return num_bodies_; }
    auto num_systems() const noexcept { return num_systems_; }

    // upload a state, evaluate it and assign every system's first levels (what starts a run)
    auto set_state(std::span<const T> positions, std::span<const T> velocities) -> void {
        pos_.upload(positions);
        vel_.upload(velocities);
        if constexpr (Order == 6) {
            hip_check(Calls::init.fn(pos_.data(), vel_.data(), acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), ticks_.data(), levels_.data(), status_.data(), workspace_.data(),
                                     workspace_bytes_, n(), b(), softening_sq_, nullptr, &params_, nullptr), Calls::init.name);
        } else {
            hip_check(Calls::init.fn(pos_.data(), vel_.data(), acc_.data(), jerk_.data(), ticks_.data(), levels_.data(), status_.data(), workspace_.data(), workspace_bytes_, n(), b(),
                                     softening_sq_, nullptr, &params_, nullptr), Calls::init.name);
        }
    }

    // one block step of every system whose next one does not pass t_stop
    auto step(double t_stop, nb_stream_t stream = nullptr) -> void {
        if constexpr (Order == 6) {
            hip_check(Calls::step.fn(pos_.data(), vel_.data(), acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), ticks_.data(), levels_.data(), status_.data(), workspace_.data(),
                                     workspace_bytes_, n(), b(), softening_sq_, nullptr, &params_, t_stop, stream), Calls::step.name);
        } else {
            hip_check(Calls::step.fn(pos_.data(), vel_.data(), acc_.data(), jerk_.data(), ticks_.data(), levels_.data(), status_.data(), workspace_.data(), workspace_bytes_, n(), b(),
                                     softening_sq_, nullptr, &params_, t_stop, stream), Calls::step.name);
        }
    }

    // the status records folded on the device, then 64 bytes read (waits for the calls before it)
    auto summary(nb_stream_t stream = nullptr) -> nb_hermite_block_ensemble_summary_t {
        hip_check(Calls::summary.fn(status_.data(), b(), summary_.data(), stream), Calls::summary.name);
        nb_hermite_block_ensemble_summary_t out{};
        summary_.download(std::span<nb_hermite_block_ensemble_summary_t>(&out, 1));
        return out;
    }
    auto statuses() const -> std::vector<nb_hermite_block_status_t> {
        auto out = std::vector<nb_hermite_block_status_t>(num_systems_);
        status_.download(out);
        return out;
    }

    // block steps until every system's next one would pass t_stop: batches of calls and one summary, 64 bytes read between them
    auto advance(double t_stop, int batch = 64) -> nb_hermite_block_ensemble_summary_t {
        for (;;) {
            for (int i = 0; i < batch; ++i) step(t_stop);
            const auto now = summary();
            if (now.stopped == now.systems) return now;
        }
    }

    // every body predicted to its system's status time -> get_positions(), get_velocities()
    auto sync(nb_stream_t stream = nullptr) -> void {
        if constexpr (Order == 6) {
            hip_check(Calls::sync.fn(pos_out_.data(), vel_out_.data(), pos_.data(), vel_.data(), acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), ticks_.data(), status_.data(), n(), b(),
                                     &params_, stream), Calls::sync.name);
        } else {
            hip_check(Calls::sync.fn(pos_out_.data(), vel_out_.data(), pos_.data(), vel_.data(), acc_.data(), jerk_.data(), ticks_.data(), status_.data(), n(), b(), &params_, stream),
                      Calls::sync.name);
        }
    }
    auto get_positions(std::span<T> out) const -> void { pos_out_.download(out); }
    auto get_velocities(std::span<T> out) const -> void { vel_out_.download(out); }
    // the snapshot of the last sync() on the device (T[4*N*B] each, for a diagnostic that reads it in place)
    auto positions_device() const noexcept -> const T* { return pos_out_.data(); }
    auto velocities_device() const noexcept -> const T* { return vel_out_.data(); }

 private:
    auto n() const noexcept { return static_cast<unsigned>(num_bodies_); }
    auto b() const noexcept { return static_cast<unsigned>(num_systems_); }
    std::size_t                                      num_bodies_, num_systems_;
    T                                                softening_sq_;
    nb_hermite_block_params_t                        params_;
    std::size_t                                      workspace_bytes_ = 0;
    DeviceArray<T>                                   pos_, vel_, acc_, jerk_, snap_, crackle_, pos_out_, vel_out_;  // (snap_ and crackle_ stay empty at 4th order)
    DeviceArray<std::uint64_t>                       ticks_;
    DeviceArray<std::int32_t>                        levels_;
    DeviceArray<nb_hermite_block_status_t>           status_;
    DeviceArray<nb_hermite_block_ensemble_summary_t> summary_;
    DeviceArray<unsigned char>                       workspace_;
};

template <std::floating_point T> using BodyEnsembleHIPHermiteBlock  = BodyEnsembleHIPHermiteBlockOrder<T, 4>;
template <std::floating_point T> using BodyEnsembleHIPHermite6Block = BodyEnsembleHIPHermiteBlockOrder<T, 6>;
