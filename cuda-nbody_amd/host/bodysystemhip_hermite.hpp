// bodysystemhip_hermite.hpp -- BodySystemHIPHermiteOrder<T, Order>: one system of N bodies on the device, stepped by the 4th-order
// Hermite scheme of nb_hermite_* (include/nbody_hip_hermite.h, libnbody_hip_hermite.so) or the 6th-order one of nb_hermite6_*
// (include/nbody_hip_hermite6.h, libnbody_hip_hermite6.so); BodySystemHIPHermite<T> and BodySystemHIPHermite6<T> name the two.
// Positions (stepped in place: the call allows new == old), velocities, accelerations, jerks, at 6th order snaps and crackles, and the
// workspace are DeviceArrays (a device without room throws DeviceBadAlloc).  A refused call throws std::runtime_error carrying the
// nb_error_string name.
#pragma once

#include "device_array.hpp"
#include "hermite_calls.hpp"

#include <concepts>
#include <cstddef>
#include <span>

template <std::floating_point T, int Order> class BodySystemHIPHermiteOrder {
    using Calls = HermiteCalls<T, Order>;

 public:
    BodySystemHIPHermiteOrder(std::size_t num_bodies, T softening_sq) : num_bodies_(num_bodies), softening_sq_(softening_sq) {
        // the sizes the step refuses are refused here, before anything is allocated
        std::size_t bytes = 0;
        hip_check(num_bodies <= 0xFFFFFFFFu ? Calls::workspace_bytes.fn(static_cast<unsigned>(num_bodies), sizeof(T), &bytes) : NB_ERR_INVALID_ARGUMENT, Calls::workspace_bytes.name);
        pos_  = DeviceArray<T>(4 * num_bodies);
        vel_  = DeviceArray<T>(4 * num_bodies);
        acc_  = DeviceArray<T>(4 * num_bodies);
        jerk_ = DeviceArray<T>(4 * num_bodies);
        if constexpr (Order == 6) {
            snap_    = DeviceArray<T>(4 * num_bodies);
            crackle_ = DeviceArray<T>(4 * num_bodies);
        }
        workspace_ = DeviceArray<T>(bytes / sizeof(T));
    }

    auto num_bodies() const noexcept { return num_bodies_; }
    auto positions() const noexcept -> const T* { return pos_.data(); }
    auto velocities() const noexcept -> const T* { return vel_.data(); }

    // upload a state and evaluate its accelerations and jerks, at 6th order its snaps too, the crackles starting at 0 (what starts a run)
    auto set_state(std::span<const T> positions, std::span<const T> velocities) -> void {
        pos_.upload(positions);
        vel_.upload(velocities);
        const auto n     = static_cast<unsigned>(num_bodies_);
        const auto bytes = workspace_.size() * sizeof(T);
        if constexpr (Order == 6) {
            hip_check(Calls::init.fn(acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), pos_.data(), vel_.data(), workspace_.data(), bytes, n, softening_sq_, nullptr), Calls::init.name);
        } else {
            hip_check(Calls::eval.fn(acc_.data(), jerk_.data(), pos_.data(), vel_.data(), n, softening_sq_, nullptr), Calls::eval.name);
        }
    }
    auto get_positions(std::span<T> out) const -> void { pos_.download(out); }
    auto get_velocities(std::span<T> out) const -> void { vel_.download(out); }

    auto update(T dt, nb_stream_t stream = nullptr) -> void {
        const auto n     = static_cast<unsigned>(num_bodies_);
        const auto bytes = workspace_.size() * sizeof(T);
        if constexpr (Order == 6) {
            hip_check(Calls::step.fn(pos_.data(), pos_.data(), vel_.data(), acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), workspace_.data(), bytes, n, dt, softening_sq_, stream), Calls::step.name);
        } else {
            hip_check(Calls::step.fn(pos_.data(), pos_.data(), vel_.data(), acc_.data(), jerk_.data(), workspace_.data(), bytes, n, dt, softening_sq_, stream), Calls::step.name);
        }
    }

 private:
    std::size_t    num_bodies_;
    T              softening_sq_;
    DeviceArray<T> pos_, vel_, acc_, jerk_, snap_, crackle_, workspace_;  // (snap_ and crackle_ stay empty at 4th order)
};

template <std::floating_point T> using BodySystemHIPHermite  = BodySystemHIPHermiteOrder<T, 4>;
template <std::floating_point T> using BodySystemHIPHermite6 = BodySystemHIPHermiteOrder<T, 6>;
