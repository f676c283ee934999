// field_cli.hpp -- `nbody --field=<file>`: after a run, the acceleration and the potential of the final state at the points of a text
// file (FieldProbeHIP, libnbody_hip_field.so).
#pragma once

#include <cstddef>
#include <filesystem>
#include <span>
#include <string>
#include <vector>

inline constexpr std::size_t kFieldMaxPoints = 65536;

// The file is text, one point `x y z` per line; `#` starts a comment, blank lines are skipped; 1 to 65 536 points, every coordinate
// finite.  -> the error message, empty when `points` holds x y z of every point in file order.
auto read_field_points(const std::filesystem::path& file, std::vector<double>& points) -> std::string;

// Prints one line per point, in file order (softened as the run, nobody excluded):
//   field at (x, y, z): acceleration (ax, ay, az), potential P
auto report_field(std::span<const float> positions, std::span<const double> points, float softening_sq) -> void;
auto report_field(std::span<const double> positions, std::span<const double> points, double softening_sq) -> void;
