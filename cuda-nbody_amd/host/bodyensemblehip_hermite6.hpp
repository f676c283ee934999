// bodyensemblehip_hermite6.hpp -- BodyEnsembleHIPHermite6<T>: B independent systems of N bodies on the device, stepped together by the
// 6th-order Hermite scheme of nb_hermite6_ensemble_* (include/nbody_hip_hermite6_ensemble.h, libnbody_hip_hermite6_ensemble.so), with one
// time step for all (update) or a clock per system (begin / advance): BodyEnsembleHIPHermite's interface (bodyensemblehip_hermite.hpp)
// with snaps and crackles beside the accelerations and jerks.  A refused call throws std::runtime_error carrying the nb_error_string name.
#pragma once

#include "../../include/nbody_hip_hermite6_ensemble.h"
#include "device_array.hpp"

#include <concepts>
#include <cstddef>
#include <span>
#include <vector>

template <std::floating_point T> class BodyEnsembleHIPHermite6 {
 public:
    BodyEnsembleHIPHermite6(std::size_t num_bodies, std::size_t num_systems, T softening_sq) : num_bodies_(num_bodies), num_systems_(num_systems), softening_sq_(softening_sq) {
        // the sizes the step refuses are refused here, before anything is allocated
        std::size_t bytes = 0;
        const bool  fits  = num_bodies <= 0xFFFFFFFFu && num_systems <= 0xFFFFFFFFu;
        hip_check(fits ? nb_hermite6_ensemble_workspace_bytes(static_cast<unsigned>(num_bodies), static_cast<unsigned>(num_systems), sizeof(T), &bytes) : NB_ERR_INVALID_ARGUMENT,
                  "nb_hermite6_ensemble_workspace_bytes");
        const auto elements = 4 * num_bodies * num_systems;
        pos_       = DeviceArray<T>(elements);
        vel_       = DeviceArray<T>(elements);
        acc_       = DeviceArray<T>(elements);
        jerk_      = DeviceArray<T>(elements);
        snap_      = DeviceArray<T>(elements);
        crackle_   = DeviceArray<T>(elements);
        workspace_ = DeviceArray<unsigned char>(bytes);
        clocks_    = DeviceArray<nb_hermite_ensemble_clock_t>(num_systems);
        status_    = DeviceArray<nb_hermite_ensemble_status_t>(1);
    }

    auto num_bodies() const noexcept { return num_bodies_; }
    auto num_systems() const noexcept { return num_systems_; }

    // upload a state and evaluate its accelerations, jerks and snaps; crackles 0 (what starts a run with one time step for all)
    auto set_state(std::span<const T> positions, std::span<const T> velocities) -> void {
        pos_.upload(positions);
        vel_.upload(velocities);
        int status;
        if constexpr (sizeof(T) == 4) {
            status = nb_hermite6_ensemble_init_f32(acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), pos_.data(), vel_.data(), workspace_.data(), workspace_.size(), n(), b(), softening_sq_, nullptr, nullptr);
        } else {
            status = nb_hermite6_ensemble_init_f64(acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), pos_.data(), vel_.data(), workspace_.data(), workspace_.size(), n(), b(), softening_sq_, nullptr, nullptr);
        }
        hip_check(status, "nb_hermite6_ensemble_init");
    }
    auto get_positions(std::span<T> out) const -> void { pos_.download(out); }
    auto get_velocities(std::span<T> out) const -> void { vel_.download(out); }

    // one step of every system with the same dt
    auto update(T dt, nb_stream_t stream = nullptr) -> void {
        int status;
        if constexpr (sizeof(T) == 4) {
            status = nb_hermite6_ensemble_step_f32(pos_.data(), pos_.data(), vel_.data(), acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), workspace_.data(), workspace_.size(), n(), b(), dt, softening_sq_, nullptr, stream);
        } else {
            status = nb_hermite6_ensemble_step_f64(pos_.data(), pos_.data(), vel_.data(), acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), workspace_.data(), workspace_.size(), n(), b(), dt, softening_sq_, nullptr, stream);
        }
        hip_check(status, "nb_hermite6_ensemble_step");
    }

    // the adaptive form: the derivatives and the clocks of the uploaded state, then one step per call of every system that can still move
    auto begin(T eta, nb_stream_t stream = nullptr) -> void {
        int status;
        if constexpr (sizeof(T) == 4) {
            status = nb_hermite6_ensemble_begin_f32(acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), pos_.data(), vel_.data(), clocks_.data(), n(), b(), softening_sq_, nullptr, eta, workspace_.data(), workspace_.size(), stream);
        } else {
            status = nb_hermite6_ensemble_begin_f64(acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), pos_.data(), vel_.data(), clocks_.data(), n(), b(), softening_sq_, nullptr, eta, workspace_.data(), workspace_.size(), stream);
        }
        hip_check(status, "nb_hermite6_ensemble_begin");
    }
    auto advance(double t_stop, double dt_max, T eta, nb_stream_t stream = nullptr) -> void {
        int status;
        if constexpr (sizeof(T) == 4) {
            status = nb_hermite6_ensemble_advance_f32(pos_.data(), pos_.data(), vel_.data(), acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), clocks_.data(), status_.data(), workspace_.data(),
                                                      workspace_.size(), n(), b(), t_stop, dt_max, eta, softening_sq_, nullptr, stream);
        } else {
            status = nb_hermite6_ensemble_advance_f64(pos_.data(), pos_.data(), vel_.data(), acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), clocks_.data(), status_.data(), workspace_.data(),
                                                      workspace_.size(), n(), b(), t_stop, dt_max, eta, softening_sq_, nullptr, stream);
        }
        hip_check(status, "nb_hermite6_ensemble_advance");
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
    DeviceArray<T>                            pos_, vel_, acc_, jerk_, snap_, crackle_;
    DeviceArray<unsigned char>                workspace_;
    DeviceArray<nb_hermite_ensemble_clock_t>  clocks_;
    DeviceArray<nb_hermite_ensemble_status_t> status_;
};
