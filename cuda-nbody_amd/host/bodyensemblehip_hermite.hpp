// bodyensemblehip_hermite.hpp -- BodyEnsembleHIPHermiteOrder<T, Order>: B independent systems of N bodies on the device, stepped together
// by the 4th-order Hermite scheme of nb_hermite_ensemble_* (include/nbody_hip_hermite_ensemble.h, libnbody_hip_hermite_ensemble.so) or the
// 6th-order one of nb_hermite6_ensemble_* (include/nbody_hip_hermite6_ensemble.h, libnbody_hip_hermite6_ensemble.so), with one time step
// for all (update) or a clock per system (begin / advance); BodyEnsembleHIPHermite<T> and BodyEnsembleHIPHermite6<T> name the two.
// Positions (stepped in place: the calls allow new == old), velocities, accelerations, jerks, at 6th order snaps and crackles, the
// workspace, the clocks and the status record are DeviceArrays (a device without room throws DeviceBadAlloc), 4*N*B T each for the
// bodies; system s holds bodies [s*N, (s+1)*N).  A refused call throws std::runtime_error carrying the nb_error_string name.
#pragma once

#include "device_array.hpp"
#include "hermite_calls.hpp"

#include <concepts>
#include <cstddef>
#include <span>
#include <vector>

template <std::floating_point T, int Order> class BodyEnsembleHIPHermiteOrder {
    using Calls = HermiteEnsembleCalls<T, Order>;

 public:
    BodyEnsembleHIPHermiteOrder(std::size_t num_bodies, std::size_t num_systems, T softening_sq) : num_bodies_(num_bodies), num_systems_(num_systems), softening_sq_(softening_sq) {
        // the sizes the step refuses are refused here, before anything is allocated
        std::size_t bytes = 0;
        const bool  fits  = num_bodies <= 0xFFFFFFFFu && num_systems <= 0xFFFFFFFFu;
        hip_check(fits ? Calls::workspace_bytes.fn(static_cast<unsigned>(num_bodies), static_cast<unsigned>(num_systems), sizeof(T), &bytes) : NB_ERR_INVALID_ARGUMENT,
                  Calls::workspace_bytes.name);
        const auto elements = 4 * num_bodies * num_systems;
        pos_  = DeviceArray<T>(elements);
        vel_  = DeviceArray<T>(elements);
        acc_  = DeviceArray<T>(elements);
        jerk_ = DeviceArray<T>(elements);
        if constexpr (Order == 6) {
            snap_    = DeviceArray<T>(elements);
            crackle_ = DeviceArray<T>(elements);
        }
        workspace_ = DeviceArray<unsigned char>(bytes);
        clocks_    = DeviceArray<nb_hermite_ensemble_clock_t>(num_systems);
        status_    = DeviceArray<nb_hermite_ensemble_status_t>(1);
    }

    auto num_bodies() const noexcept { return num_bodies_; }
    auto num_systems() const noexcept { return num_systems_; }

    // upload a state and evaluate its accelerations and jerks, at 6th order its snaps too, the crackles starting at 0 (what starts a run
    // with one time step for all)
    auto set_state(std::span<const T> positions, std::span<const T> velocities) -> void {
        pos_.upload(positions);
        vel_.upload(velocities);
        if constexpr (Order == 6) {
            hip_check(Calls::init.fn(acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), pos_.data(), vel_.data(), workspace_.data(), workspace_.size(), n(), b(), softening_sq_, nullptr, nullptr),
                      Calls::init.name);
        } else {
            hip_check(Calls::eval.fn(acc_.data(), jerk_.data(), pos_.data(), vel_.data(), n(), b(), softening_sq_, nullptr, nullptr), Calls::eval.name);
        }
    }
    auto get_positions(std::span<T> out) const -> void { pos_.download(out); }
    auto get_velocities(std::span<T> out) const -> void { vel_.download(out); }
    // the current state on the device (T[4*N*B] each, for a diagnostic that reads it in place)
    auto positions_device() const noexcept -> const T* { return pos_.data(); }
    auto velocities_device() const noexcept -> const T* { return vel_.data(); }

    // one step of every system with the same dt
    auto update(T dt, nb_stream_t stream = nullptr) -> void {
        if constexpr (Order == 6) {
            hip_check(Calls::step.fn(pos_.data(), pos_.data(), vel_.data(), acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), workspace_.data(), workspace_.size(), n(), b(), dt, softening_sq_,
                                     nullptr, stream), Calls::step.name);
        } else {
            hip_check(Calls::step.fn(pos_.data(), pos_.data(), vel_.data(), acc_.data(), jerk_.data(), workspace_.data(), workspace_.size(), n(), b(), dt, softening_sq_, nullptr, stream),
                      Calls::step.name);
        }
    }

    // the adaptive form: the clocks (at 6th order the derivatives too) of the uploaded state, then one step per call of every system that
    // can still move
    auto begin(T eta, nb_stream_t stream = nullptr) -> void {
        if constexpr (Order == 6) {
            hip_check(Calls::begin.fn(acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), pos_.data(), vel_.data(), clocks_.data(), n(), b(), softening_sq_, nullptr, eta, workspace_.data(),
                                      workspace_.size(), stream), Calls::begin.name);
        } else {
            hip_check(Calls::begin.fn(acc_.data(), jerk_.data(), pos_.data(), vel_.data(), clocks_.data(), n(), b(), softening_sq_, nullptr, eta, workspace_.data(), workspace_.size(), stream),
                      Calls::begin.name);
        }
    }
    auto advance(double t_stop, double dt_max, T eta, nb_stream_t stream = nullptr) -> void {
        if constexpr (Order == 6) {
            hip_check(Calls::advance.fn(pos_.data(), pos_.data(), vel_.data(), acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), clocks_.data(), status_.data(), workspace_.data(),
                                        workspace_.size(), n(), b(), t_stop, dt_max, eta, softening_sq_, nullptr, stream), Calls::advance.name);
        } else {
            hip_check(Calls::advance.fn(pos_.data(), pos_.data(), vel_.data(), acc_.data(), jerk_.data(), clocks_.data(), status_.data(), workspace_.data(), workspace_.size(), n(), b(), t_stop,
                                        dt_max, eta, softening_sq_, nullptr, stream), Calls::advance.name);
        }
    }
    // the 64-byte record of the last advance, and the clocks (both read back: they wait for the calls before them)
    auto status() const -> nb_hermite_ensemble_status_t {
        nb_hermite_ensemble_status_t out{};
        status_.download(std::span<nb_hermite_ensemble_status_t>(&out, 1));
        return out;
    }
    auto clocks() const -> std::vector<nb_hermite_ensemble_clock_t> {
        auto out = std::vector<nb_hermite_ensemble_clock_t>(num_systems_);
        clocks_.download(out);
        return out;
    }

 private:
    auto n() const noexcept { return static_cast<unsigned>(num_bodies_); }
    auto b() const noexcept { return static_cast<unsigned>(num_systems_); }
    std::size_t                               num_bodies_, num_systems_;
    T                                         softening_sq_;
    DeviceArray<T>                            pos_, vel_, acc_, jerk_, snap_, crackle_;  // (snap_ and crackle_ stay empty at 4th order)
    DeviceArray<unsigned char>                workspace_;
    DeviceArray<nb_hermite_ensemble_clock_t>  clocks_;
    DeviceArray<nb_hermite_ensemble_status_t> status_;
};

template <std::floating_point T> using BodyEnsembleHIPHermite  = BodyEnsembleHIPHermiteOrder<T, 4>;
template <std::floating_point T> using BodyEnsembleHIPHermite6 = BodyEnsembleHIPHermiteOrder<T, 6>;
