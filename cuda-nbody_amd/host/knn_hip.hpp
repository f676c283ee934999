// knn_hip.hpp -- KnnSurveyHIP<T>: the K nearest neighbours of every body, the local densities and the structure record of states of N bodies
// through nb_knn_* (include/nbody_hip_knn.h, libnbody_hip_knn.so).  The outputs, the record, the workspace and a staging copy of the
// positions are DeviceArrays (a device without room throws DeviceBadAlloc).  A refused call throws std::runtime_error carrying the
// nb_error_string name.  Calls are asynchronous on `stream`; the getters wait for the null stream.
#pragma once

#include "../../include/nbody_hip_knn.h"
#include "device_array.hpp"

#include <concepts>
#include <cstddef>
#include <span>

template <std::floating_point T> class KnnSurveyHIP {
 public:
    KnnSurveyHIP(std::size_t num_bodies, unsigned k) : num_bodies_(num_bodies), k_(k) {
        // the sizes the calls refuse are refused here, before anything is allocated
        hip_check(num_bodies <= 0xFFFFFFFFu ? nb_knn_workspace_bytes(static_cast<unsigned>(num_bodies), k, sizeof(T), &workspace_bytes_) : NB_ERR_INVALID_ARGUMENT,
                  "nb_knn_workspace_bytes");
        pos_       = DeviceArray<T>(4 * num_bodies);
        index_     = DeviceArray<unsigned>(num_bodies * k);
        dist_sq_   = DeviceArray<T>(num_bodies * k);
        densities_ = DeviceArray<T>(num_bodies);
        structure_ = DeviceArray<nb_knn_structure_t>(1);
        workspace_ = DeviceArray<unsigned char>(workspace_bytes_);
    }

    auto num_bodies() const noexcept { return num_bodies_; }
    auto k() const noexcept { return k_; }

    // the lists and, with K >= 2, the densities and the record of the device array `positions` (T[4 N], only read)
    auto survey(const T* positions, nb_stream_t stream = nullptr) -> void {
        const auto n         = static_cast<unsigned>(num_bodies_);
        T* const   densities = k_ >= 2 ? densities_.data() : nullptr;
        auto* const record   = k_ >= 2 ? structure_.data() : nullptr;
        int         status;
        if constexpr (sizeof(T) == 4) {
            status = nb_knn_survey_f32(positions, n, k_, index_.data(), dist_sq_.data(), densities, record, workspace_.data(), workspace_bytes_, stream);
        } else {
            status = nb_knn_survey_f64(positions, n, k_, index_.data(), dist_sq_.data(), densities, record, workspace_.data(), workspace_bytes_, stream);
        }
        hip_check(status, "nb_knn_survey");
    }
    // ... of a state on the host
    auto survey(std::span<const T> positions) -> void {
        pos_.upload(positions);
        survey(pos_.data());
    }

    auto structure() const -> nb_knn_structure_t {
        nb_knn_structure_t out{};
        structure_.download(std::span<nb_knn_structure_t>(&out, 1));
        return out;
    }
    auto get_index(std::span<unsigned> out) const -> void { index_.download(out); }
    auto get_dist_sq(std::span<T> out) const -> void { dist_sq_.download(out); }
    auto get_densities(std::span<T> out) const -> void { densities_.download(out); }

 private:
    std::size_t                     num_bodies_;
    unsigned                        k_;
    std::size_t                     workspace_bytes_ = 0;
    DeviceArray<T>                  pos_, dist_sq_, densities_;
    DeviceArray<unsigned>           index_;
    DeviceArray<nb_knn_structure_t> structure_;
    DeviceArray<unsigned char>      workspace_;
};
