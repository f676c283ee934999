// bodysystemhip_hermite_block.hpp -- BodySystemHIPHermiteBlockOrder<T, Order>: one system of N bodies on the device, stepped by the
// Hermite scheme with block time steps, at 4th order by nb_hermite_block_* (include/nbody_hip_hermite_block.h,
// libnbody_hip_hermite_block.so), at 6th order by nb_hermite6_block_* (include/nbody_hip_hermite6_block.h,
// libnbody_hip_hermite6_block.so); BodySystemHIPHermiteBlock<T> and BodySystemHIPHermite6Block<T> name the two.  The state (positions,
// velocities, accelerations, jerks, at 6th order snaps and crackles, ticks, levels), the status record, the workspace and a synchronised
// snapshot are DeviceArrays (a device without room throws DeviceBadAlloc).  A refused call throws std::runtime_error carrying the
// nb_error_string name.
#pragma once

#include "device_array.hpp"
#include "hermite_calls.hpp"

#include <concepts>
#include <cstddef>
#include <cstdint>
#include <span>

template <std::floating_point T, int Order> class BodySystemHIPHermiteBlockOrder {
    using Calls = HermiteBlockCalls<T, Order>;

 public:
    BodySystemHIPHermiteBlockOrder(std::size_t num_bodies, T softening_sq, const nb_hermite_block_params_t& params) : num_bodies_(num_bodies), softening_sq_(softening_sq), params_(params) {
        // the sizes the step refuses are refused here, before anything is allocated
        hip_check(num_bodies <= 0xFFFFFFFFu ? Calls::workspace_bytes.fn(static_cast<unsigned>(num_bodies), sizeof(T), &workspace_bytes_) : NB_ERR_INVALID_ARGUMENT,
                  Calls::workspace_bytes.name);
        pos_  = DeviceArray<T>(4 * num_bodies);
        vel_  = DeviceArray<T>(4 * num_bodies);
        acc_  = DeviceArray<T>(4 * num_bodies);
        jerk_ = DeviceArray<T>(4 * num_bodies);
        if constexpr (Order == 6) {
            snap_    = DeviceArray<T>(4 * num_bodies);
            crackle_ = DeviceArray<T>(4 * num_bodies);
        }
        pos_out_   = DeviceArray<T>(4 * num_bodies);
        vel_out_   = DeviceArray<T>(4 * num_bodies);
        ticks_     = DeviceArray<std::uint64_t>(num_bodies);
        levels_    = DeviceArray<std::int32_t>(num_bodies);
        status_    = DeviceArray<nb_hermite_block_status_t>(1);
        workspace_ = DeviceArray<unsigned char>(workspace_bytes_);
    }

    auto num_bodies() const noexcept { return num_bodies_; }
    // the synchronised snapshot (after sync())
    auto positions() const noexcept -> const T* { return pos_out_.data(); }
    auto velocities() const noexcept -> const T* { return vel_out_.data(); }

    // upload a state, evaluate it and assign the first levels (what starts a run)
    auto set_state(std::span<const T> positions, std::span<const T> velocities) -> void {
        pos_.upload(positions);
        vel_.upload(velocities);
        const auto n = static_cast<unsigned>(num_bodies_);
        if constexpr (Order == 6) {
            hip_check(Calls::init.fn(pos_.data(), vel_.data(), acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), ticks_.data(), levels_.data(), status_.data(), workspace_.data(),
                                     workspace_bytes_, n, softening_sq_, &params_, nullptr), Calls::init.name);
        } else {
            hip_check(Calls::init.fn(pos_.data(), vel_.data(), acc_.data(), jerk_.data(), ticks_.data(), levels_.data(), status_.data(), workspace_.data(), workspace_bytes_, n, softening_sq_,
                                     &params_, nullptr), Calls::init.name);
        }
    }

    // one block step, or nothing but the flag when it would pass t_stop
    auto step(double t_stop, nb_stream_t stream = nullptr) -> void {
        const auto n = static_cast<unsigned>(num_bodies_);
        if constexpr (Order == 6) {
            hip_check(Calls::step.fn(pos_.data(), vel_.data(), acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), ticks_.data(), levels_.data(), status_.data(), workspace_.data(),
                                     workspace_bytes_, n, softening_sq_, &params_, t_stop, stream), Calls::step.name);
        } else {
            hip_check(Calls::step.fn(pos_.data(), vel_.data(), acc_.data(), jerk_.data(), ticks_.data(), levels_.data(), status_.data(), workspace_.data(), workspace_bytes_, n, softening_sq_,
                                     &params_, t_stop, stream), Calls::step.name);
        }
    }

    auto status() const -> nb_hermite_block_status_t {
        nb_hermite_block_status_t out{};
        status_.download(std::span<nb_hermite_block_status_t>(&out, 1));
        return out;
    }

    // block steps until the next one would pass t_stop: batches of calls, the status read between them
    auto advance(double t_stop, int batch = 64) -> nb_hermite_block_status_t {
        for (;;) {
            for (int i = 0; i < batch; ++i) step(t_stop);
            const auto now = status();
            if ((now.flags & NB_HERMITE_BLOCK_STOPPED) != 0) return now;
        }
    }

    // every body predicted to the status time -> positions(), velocities()
    auto sync(nb_stream_t stream = nullptr) -> void {
        const auto n = static_cast<unsigned>(num_bodies_);
        if constexpr (Order == 6) {
            hip_check(Calls::sync.fn(pos_out_.data(), vel_out_.data(), pos_.data(), vel_.data(), acc_.data(), jerk_.data(), snap_.data(), crackle_.data(), ticks_.data(), status_.data(), n,
                                     &params_, stream), Calls::sync.name);
        } else {
            hip_check(Calls::sync.fn(pos_out_.data(), vel_out_.data(), pos_.data(), vel_.data(), acc_.data(), jerk_.data(), ticks_.data(), status_.data(), n, &params_, stream), Calls::sync.name);
        }
    }
    auto get_positions(std::span<T> out) const -> void { pos_out_.download(out); }
    auto get_velocities(std::span<T> out) const -> void { vel_out_.download(out); }

 private:
    std::size_t                            num_bodies_;
    T                                      softening_sq_;
    nb_hermite_block_params_t              params_;
    std::size_t                            workspace_bytes_ = 0;
    DeviceArray<T>                         pos_, vel_, acc_, jerk_, snap_, crackle_, pos_out_, vel_out_;  // (snap_ and crackle_ stay empty at 4th order)
    DeviceArray<std::uint64_t>             ticks_;
    DeviceArray<std::int32_t>              levels_;
    DeviceArray<nb_hermite_block_status_t> status_;
    DeviceArray<unsigned char>             workspace_;
};

template <std::floating_point T> using BodySystemHIPHermiteBlock  = BodySystemHIPHermiteBlockOrder<T, 4>;
template <std::floating_point T> using BodySystemHIPHermite6Block = BodySystemHIPHermiteBlockOrder<T, 6>;
