// knn_cli.cpp -- `nbody --knn=<K>` (knn_cli.hpp)
#include "knn_cli.hpp"

#include "knn_hip.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>

namespace {

template <typename T> auto radii_of(std::span<const T> positions, const std::array<double, 3>& centre, std::span<const double> fractions) -> std::vector<double> {
    const auto          n = positions.size() / 4;
    std::vector<double> r(n);
    for (std::size_t i = 0; i < n; ++i) {
        const double dx = static_cast<double>(positions[4 * i]) - centre[0], dy = static_cast<double>(positions[4 * i + 1]) - centre[1],
                     dz = static_cast<double>(positions[4 * i + 2]) - centre[2];
        r[i] = std::sqrt(dx * dx + dy * dy + dz * dz);
    }
    std::vector<std::size_t> order(n);
    std::iota(order.begin(), order.end(), std::size_t{0});
    std::stable_sort(order.begin(), order.end(), [&](std::size_t a, std::size_t b) { return r[a] < r[b]; });
    std::vector<double> cumulative(n);
    double              mass = 0.0;
    for (std::size_t s = 0; s < n; ++s) cumulative[s] = mass += static_cast<double>(positions[4 * order[s] + 3]);
    std::vector<double> out;
    for (const double f : fractions) {
        const auto at = static_cast<std::size_t>(std::lower_bound(cumulative.begin(), cumulative.end(), f * mass) - cumulative.begin());
        out.push_back(n == 0 ? 0.0 : r[order[std::min(at, n - 1)]]);
    }
    return out;
}

template <typename T> auto report(std::span<const T> positions, unsigned k) -> void {
    const auto n      = positions.size() / 4;
    auto       survey = KnnSurveyHIP<T>(n, k);
    survey.survey(positions);
    const auto s     = survey.structure();
    const bool dense = (s.flags & NB_KNN_NO_DENSITY) == 0;
    if (dense) {
        std::printf("density centre: %.17g %.17g %.17g (K = %u, %u bodies defined, %u degenerate)\n", s.centre[0], s.centre[1], s.centre[2], k, s.defined, s.degenerate);
    } else {
        std::printf("density centre: none (K = %u, %u bodies defined, %u degenerate)\n", k, s.defined, s.degenerate);
    }
    std::printf("density radius: %.17g, core radius: %.17g\n", s.density_radius, s.core_radius);
    std::printf("densest body: %u, density %.17g\n", s.max_density_body, s.max_density);
    std::printf("K-th neighbour distance: smallest %.17g, largest %.17g\n", std::sqrt(s.min_kth_dist_sq), std::sqrt(s.max_kth_dist_sq));
    if (dense) {
        const double fractions[] = {0.1, 0.5, 0.9};
        const auto   radii       = radii_of<T>(positions, {s.centre[0], s.centre[1], s.centre[2]}, fractions);
        std::printf("Lagrangian radii (10%%, 50%%, 90%%): %.17g %.17g %.17g\n", radii[0], radii[1], radii[2]);
    }
}

}  // namespace

auto report_knn(std::span<const float> positions, unsigned k) -> void { report<float>(positions, k); }
auto report_knn(std::span<const double> positions, unsigned k) -> void { report<double>(positions, k); }

auto lagrangian_radii(std::span<const float> positions, const std::array<double, 3>& centre, std::span<const double> fractions) -> std::vector<double> {
    return radii_of<float>(positions, centre, fractions);
}
auto lagrangian_radii(std::span<const double> positions, const std::array<double, 3>& centre, std::span<const double> fractions) -> std::vector<double> {
    return radii_of<double>(positions, centre, fractions);
}
