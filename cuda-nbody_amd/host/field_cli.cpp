// field_cli.cpp -- `nbody --field=<file>` (field_cli.hpp)
#include "field_cli.hpp"

#include "field_hip.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>

auto read_field_points(const std::filesystem::path& file, std::vector<double>& points) -> std::string {
    points.clear();
    if (!std::filesystem::is_regular_file(file)) return "--field: File does not exist: " + file.string();
    auto in = std::ifstream(file);
    if (!in) return "--field: cannot open " + file.string();
    std::string line;
    std::size_t number = 0;
    while (std::getline(in, line)) {
        ++number;
        if (const auto hash = line.find('#'); hash != std::string::npos) line.erase(hash);
        if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
        const auto where = file.string() + ":" + std::to_string(number);
        double      xyz[3];
        const char* at = line.c_str();
        for (auto& coordinate : xyz) {
            char* end  = nullptr;
            coordinate = std::strtod(at, &end);
            if (end == at) return "--field: " + where + ": expected three numbers `x y z`";
            if (!std::isfinite(coordinate)) return "--field: " + where + ": a coordinate is not finite";
            at = end;
        }
        if (std::string(at).find_first_not_of(" \t\r") != std::string::npos) return "--field: " + where + ": expected three numbers `x y z`";
        if (points.size() / 3 == kFieldMaxPoints) return "--field: " + file.string() + " holds more than 65536 points";
        points.insert(points.end(), xyz, xyz + 3);
    }
    if (points.empty()) return "--field: " + file.string() + " holds no point";
    return {};
}

namespace {

template <typename T> auto report(std::span<const T> positions, std::span<const double> points, T softening_sq) -> void {
    const auto     n = positions.size() / 4, m = points.size() / 3;
    std::vector<T> targets(4 * m, T(0));
    for (std::size_t k = 0; k < m; ++k) {
        for (int c = 0; c < 3; ++c) targets[4 * k + c] = static_cast<T>(points[3 * k + c]);
    }
    auto probe = FieldProbeHIP<T>(n, m);
    probe.eval(positions, std::span<const T>(targets), softening_sq);
    std::vector<T> acc(4 * m), potentials(m);
    probe.get_accelerations(acc);
    probe.get_potentials(potentials);
    for (std::size_t k = 0; k < m; ++k) {
        std::printf("field at (%.9g, %.9g, %.9g): acceleration (%.9g, %.9g, %.9g), potential %.9g\n", static_cast<double>(targets[4 * k]), static_cast<double>(targets[4 * k + 1]),
                    static_cast<double>(targets[4 * k + 2]), static_cast<double>(acc[4 * k]), static_cast<double>(acc[4 * k + 1]), static_cast<double>(acc[4 * k + 2]),
                    static_cast<double>(potentials[k]));
    }
}

}  // namespace

auto report_field(std::span<const float> positions, std::span<const double> points, float softening_sq) -> void { report<float>(positions, points, softening_sq); }
auto report_field(std::span<const double> positions, std::span<const double> points, double softening_sq) -> void { report<double>(positions, points, softening_sq); }
