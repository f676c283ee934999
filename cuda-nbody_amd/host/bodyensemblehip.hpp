// bodyensemblehip.hpp -- BodyEnsembleHIP<T>: B independent systems of N bodies on the device, stepped together by
// nb_ensemble_integrate_* (include/nbody_hip_ensemble.h, libnbody_hip_ensemble.so).  The storage of BodySystemHIP (two ping-pong
// position arrays + one velocity array, DeviceArray: a device without room throws DeviceBadAlloc), for 4*N*B T each; system s
// holds bodies [s*N, (s+1)*N).  A refused call throws std::runtime_error carrying the nb_error_string name.
#pragma once

#include "../../include/nbody_hip_ensemble.h"
#include "device_array.hpp"

#include <concepts>
#include <cstddef>
#include <span>

template <std::floating_point T> class BodyEnsembleHIP {
 public:
    BodyEnsembleHIP(std::size_t num_bodies, std::size_t num_systems, int mode) : num_bodies_(num_bodies), num_systems_(num_systems), mode_(mode) {
        // the sizes the step refuses are refused here, before anything is allocated
        nb_ensemble_plan_t plan{};
        const bool fits = num_bodies <= 0xFFFFFFFFu && num_systems <= 0xFFFFFFFFu;
        hip_check(fits ? plan_fn(static_cast<unsigned>(num_bodies), static_cast<unsigned>(num_systems), &plan) : NB_ERR_INVALID_ARGUMENT, "nb_ensemble_plan");
        const auto elements = 4 * num_bodies * num_systems;
        pos_[0] = DeviceArray<T>(elements);
        pos_[1] = DeviceArray<T>(elements);
        vel_    = DeviceArray<T>(elements);
    }

    auto num_bodies() const noexcept { return num_bodies_; }
    auto num_systems() const noexcept { return num_systems_; }

    auto set_positions(std::span<const T> data) -> void {
        read_ = 0;
        pos_[0].upload(data);
    }
    auto set_velocities(std::span<const T> data) -> void {
        read_ = 0;
        vel_.upload(data);
    }
    auto get_positions(std::span<T> out) const -> void { pos_[read_].download(out); }
    auto get_velocities(std::span<T> out) const -> void { vel_.download(out); }
    // the current state on the device (T[4*N*B] each, for a diagnostic that reads it in place)
    auto positions_device() const noexcept -> const T* { return pos_[read_].data(); }
    auto velocities_device() const noexcept -> const T* { return vel_.data(); }

    // One step of every system: new positions into the other array, then the two swap.  `device_params`: null (every system uses
    // dt, damping, softening_sq) or a device array T[4*B] of {dt, damping, softening^2, -} per system.
    auto update(T dt, T damping, T softening_sq, const T* device_params = nullptr, nb_stream_t stream = nullptr) -> void {
        const auto n = static_cast<unsigned>(num_bodies_), b = static_cast<unsigned>(num_systems_);
        int status;
        if constexpr (sizeof(T) == 4) {
            status = nb_ensemble_integrate_f32(pos_[1 - read_].data(), pos_[read_].data(), vel_.data(), n, b, dt, damping, softening_sq, device_params, mode_, stream);
        } else {
            status = nb_ensemble_integrate_f64(pos_[1 - read_].data(), pos_[read_].data(), vel_.data(), n, b, dt, damping, softening_sq, device_params, mode_, stream);
        }
        hip_check(status, "nb_ensemble_integrate");
        read_ = 1 - read_;
    }

 private:
    static auto plan_fn(unsigned n, unsigned b, nb_ensemble_plan_t* p) -> int {
        if constexpr (sizeof(T) == 4) return nb_ensemble_plan_f32(n, b, p); else return nb_ensemble_plan_f64(n, b, p);
    }
    std::size_t    num_bodies_, num_systems_;
    int            mode_;
    DeviceArray<T> pos_[2], vel_;
    unsigned       read_ = 0;
};
