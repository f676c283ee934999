// bodysystemhip_hermite6.hpp -- BodySystemHIPHermite6<T>: one system of N bodies on the device, stepped by the 6th-order Hermite
// scheme of nb_hermite6_* (include/nbody_hip_hermite6.h, libnbody_hip_hermite6.so).  The mirror of BodySystemHIPHermite: positions
// (stepped in place: the call allows new == old), velocities, accelerations, jerks, snaps, crackles and the workspace are DeviceArrays
// (a device without room throws DeviceBadAlloc).  A refused call throws std::runtime_error carrying the nb_error_string name.
#pragma once

#include "../../include/nbody_hip_hermite6.h"
#include "device_array.hpp"

#include <concepts>
#include <cstddef>
#include <span>

template <std::floating_point T> class BodySystemHIPHermite6 {
 public:
    BodySystemHIPHermite6(std::size_t num_bodies, T softening_sq) : num_bodies_(num_bodies), softening_sq_(softening_sq) {
        // the sizes the step refuses are refused here, before anything is allocated
        std::size_t bytes = 0;
        hip_check(num_bodies <= 0xFFFFFFFFu ? nb_hermite6_workspace_bytes(static_cast<unsigned>(num_bodies), sizeof(T), &bytes) : NB_ERR_INVALID_ARGUMENT, "nb_hermite6_workspace_bytes");
        pos_       = DeviceArray<T>(4 * num_bodies);
        vel_       = DeviceArray<T>(4 * num_bodies);
        acc_       = DeviceArray<T>(4 * num_bodies);
        jerk_      = DeviceArray<T>(4 * num_bodies);
        snap_      = DeviceArray<T>(4 * num_bodies);
        crackle_   = DeviceArray<T>(4 * num_bodies);
        workspace_ = DeviceArray<T>(bytes / sizeof(T));
    }

    auto num_bodies() const noexcept { return num_bodies_; }
    auto positions() const noexcept -> const T* { return pos_.data(); }
    auto velocities() const noexcept -> const T* { return vel_.data(); }

    // upload a state and evaluate its accelerations, jerks and snaps; the crackles start at 0 (what starts a run)
    auto set_state(std::span<const T> positions, std::span<const T> velocities) -> void {
        pos_.upload(positions);
        vel_.upload(velocities);
        const auto n     = static_cast<unsigned>(num_bodies_);
        const auto bytes = workspace_.size() * sizeof(T);
        if constexpr (sizeof(T) == 4) {
            hip_check(nb_hermite6_init_f32(acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), pos_.data(), vel_.data(), workspace_.data(), bytes, n, softening_sq_, nullptr), "nb_hermite6_init");
        } else {
            hip_check(nb_hermite6_init_f64(acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), pos_.data(), vel_.data(), workspace_.data(), bytes, n, softening_sq_, nullptr), "nb_hermite6_init");
        }
    }
    auto get_positions(std::span<T> out) const -> void { pos_.download(out); }
    auto get_velocities(std::span<T> out) const -> void { vel_.download(out); }

    auto update(T dt, nb_stream_t stream = nullptr) -> void {
        const auto n     = static_cast<unsigned>(num_bodies_);
        const auto bytes = workspace_.size() * sizeof(T);
        int        status;
        if constexpr (sizeof(T) == 4) {
            status = nb_hermite6_step_f32(pos_.data(), pos_.data(), vel_.data(), acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), workspace_.data(), bytes, n, dt, softening_sq_, stream);
        } else {
            status = nb_hermite6_step_f64(pos_.data(), pos_.data(), vel_.data(), acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), workspace_.data(), bytes, n, dt, softening_sq_, stream);
        }
        hip_check(status, "nb_hermite6_step");
    }

 private:
    std::size_t    num_bodies_;
    T              softening_sq_;
    DeviceArray<T> pos_, vel_, acc_, jerk_, snap_, crackle_, workspace_;
};
