// nbody.cpp -- command line of the MI355X N-body hot path.  Flag names, defaults, banner/benchmark output and
// exit codes follow the reference's main (/root/reference/src/nbody.cpp:254-409); the OpenGL viewer is out of
// scope, so a run needs --benchmark, --compare/--qatest or --steps.
//
//   reference flags : --fullscreen --fp64 --hostmem --benchmark --numbodies=<n> --compare --qatest --cpu
//                     --tipsy=<file> -i,--iterations=<n> --blockSize=<n>      (single-dash spellings accepted too)
//   extensions      : --numdevices=<n> | --devices=<list> (the NVIDIA sample's -numdevices, which this fork of it dropped)
//                     --mode=fast|strict  --config=shell|random|expand  --demo=<0..6>  --steps=<n>  --dump=<file>
//                     --seed=<n>  --graph  --no-workspace  --workspace-mib=<n>  --energy  --neighbours=<radius>  --knn=<K>  --field=<file>  --inject-error=<x> (test hook for --compare)  --alloc-limit-mib=<n> (test hook)
//                     --systems=<B> (B independent systems of --numbodies bodies in one launch: libnbody_hip_ensemble.so)
//                     --energies (with --systems: every system's energy at the start and the end in one call each: libnbody_hip_energy_ensemble.so)
//                     --integrator=hermite (4th-order Hermite steps: libnbody_hip_hermite.so)
//                     --integrator=hermite6 (6th-order Hermite steps: libnbody_hip_hermite6.so)
//                     --integrator=hermite-block (... with block time steps: libnbody_hip_hermite_block.so)
//                     --integrator=hermite6-block (6th-order Hermite steps with block time steps: libnbody_hip_hermite6_block.so)
//                     --integrator=hermite-ensemble --systems=<B> (... of B systems, a time step per system: libnbody_hip_hermite_ensemble.so)
//                     --integrator=hermite-block-ensemble --systems=<B> (block time steps of B systems: libnbody_hip_hermite_block_ensemble.so)
//                     --integrator=hermite6-ensemble --systems=<B> (6th-order steps of B systems, a time step per system: libnbody_hip_hermite6_ensemble.so)
//                     --integrator=hermite6-block-ensemble --systems=<B> (6th-order block time steps of B systems: libnbody_hip_hermite6_block_ensemble.so)
#include "ensemble_cli.hpp"
#include "hermite_cli.hpp"
#include "../../include/nbody_hip_hermite.h"
#include "../../include/nbody_hip_hermite6.h"
#include "../../include/nbody_hip_hermite_block.h"
#include "../../include/nbody_hip_hermite_block_ensemble.h"
#include "../../include/nbody_hip_hermite_ensemble.h"
#include "../../include/nbody_hip_knn.h"
#include "../../include/nbody_hip_neighbour.h"
#include "compute.hpp"
#include "field_cli.hpp"
#include "integrate_nbody_hip.hpp"
#include "knn_cli.hpp"
#include "neighbour_cli.hpp"

#include <dlfcn.h>  // (the --alloc-limit-mib test hook lives in the lab library: looked up, never linked)

#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <limits>
#include <new>
#include <optional>
#include <stdexcept>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

namespace {

enum class Status { OK = 0, CleanShutDown, InvalidArguments };

// --eta of --integrator=hermite6-ensemble where none is given (the largest of 0.8, 0.4, 0.2, ... that ends 5.7's binary
// system with at most half the energy error of hermite-ensemble's 0.02, in fewer steps)
constexpr double kHermite6EnsembleEta = 0.025;

struct Options {
    bool                  fullscreen = false;
    bool                  fp64       = false;
    bool                  hostmem    = false;
    bool                  benchmark  = false;
    std::size_t           numbodies  = 0;
    bool                  compare    = false;
    bool                  qatest     = false;
    bool                  cpu        = false;
    std::filesystem::path tipsy;
    std::size_t           iterations = 10;
    int                   block_size = 256;
    // extensions
    int                   mode   = NB_MODE_FAST;
    NBodyConfig           config = NBodyConfig::NBODY_CONFIG_SHELL;
    std::size_t           steps  = 0;
    std::filesystem::path dump;
    std::optional<unsigned> seed;
    bool                  graph = false;
    bool                  no_workspace = false;
    bool                  energy = false;  // print the energy at the start and the end of a --benchmark / --steps run
    bool                  energies = false;  // --systems: print what the run did to the energy of every system (the start, the drift at the end)
    std::optional<double> neighbours;  // --neighbours=<radius>: after the run, the closest pair, the neighbour counts within the radius, the deepest potential
    std::optional<unsigned> knn;  // --knn=<K>: after the run, the density centre, the density and core radii, the densest body, the Lagrangian radii
    std::vector<double>   field_points;  // --field=<file>: x y z of the points where the final state's acceleration and potential are printed
    std::size_t           workspace_mib = 0;  // 0: no bound of our own
    std::size_t           alloc_limit_mib = 0;  // test hook: device allocations above this are refused (0: none)
    std::vector<int>      devices;  // --numdevices=<n> (devices 0..n-1) or --devices=<a,b,...>: bodies sharded over several GPUs
    std::optional<std::size_t> demo;   // row of Compute::demo_params (the reference reaches them from the viewer's keys only)
    double                inject_error = 0.0;
    std::size_t           systems = 0;  // --systems=<B>: an ensemble of B systems (0: one system, the reference's run)
    bool                  hermite = false;  // --integrator=hermite or hermite-block (euler, the reference's step, is the default)
    bool                  hermite_block = false;  // --integrator=hermite-block
    bool                  hermite6 = false;  // --integrator=hermite6 (`hermite` is set too: its restrictions and messages apply)
    bool                  hermite6_block = false;  // --integrator=hermite6-block (`hermite` and `hermite_block` are set too: their restrictions, options and messages apply)
    bool                  hermite_ensemble = false;  // --integrator=hermite-ensemble (with --systems)
    bool                  hermite_block_ensemble = false;  // --integrator=hermite-block-ensemble (with --systems)
    bool                  hermite6_ensemble = false;  // --integrator=hermite6-ensemble (`hermite_ensemble` is set too: its restrictions, options and messages apply)
    bool                  hermite6_block_ensemble = false;  // --integrator=hermite6-block-ensemble (`hermite_block_ensemble` is set too: its restrictions, options and messages apply)
    std::optional<double> eta;     // --eta (hermite-block, hermite-ensemble, hermite-block-ensemble)
    std::optional<double> t_end;   // --t-end (hermite-ensemble, hermite-block-ensemble)
    std::optional<int>    levels;  // --levels (hermite-block, hermite-block-ensemble)
};

constexpr auto help_text = R"(The MI355X NBody hot path (drop-in for cuda-nbody's compute path).
Usage: nbody [OPTIONS]

Options:
  -h,--help                   Print this help message and exit
  --fullscreen                Accepted for compatibility; there is no viewer on a headless accelerator
  --fp64                      Use double precision floating point values for simulation
  --hostmem                   Stores simulation data in host memory
  --benchmark                 Run benchmark to measure performance
  --numbodies UINT            Number of bodies (>= 1) to run in simulation
  --compare                   Compares the fast kernels with the bit-reproducing strict kernels (the CPU path's arithmetic)
  --qatest                    Runs a QA test
  --cpu                       Rejected: the CPU BodySystem path is test infrastructure (oracle/), not part of this build
  --tipsy TEXT:FILE           Load a tipsy model file for simulation
  -i,--iterations UINT [10]   Number of iterations to run in the benchmark
  --blockSize INT [256]       Workgroup / LDS tile size of the strict kernels (multiple of 64); a hint for the fast ones
  --mode TEXT [fast]          fast | strict (strict bit-reproduces the reference's CPU BodySystem path)
  --config TEXT [shell]       shell | random | expand initial configuration
  --numdevices UINT           Shard the bodies over GPUs 0..n-1 of this node (position tiles exchanged over RCCL / xGMI)
  --devices LIST              ... or over the GPUs in this comma-separated list
  --demo UINT                 Select row 0..6 of the demo parameter table (dt, scales, softening, damping) and reset
  --steps UINT                Advance this many steps (untimed) before --dump; with --compare: also print how far the fast
                              trajectory is from the strict one after this many steps (max / 99th percentile / median)
  --dump TEXT                 Write final positions then velocities (raw little-endian T[4N] each) to this file
  --seed UINT                 srand() this value first (the reference never seeds: default stream = seed 1)
  --graph                     --benchmark issues its (even number of) iterations as one captured hipGraph
  --no-workspace              Fast mode without scratch memory: every directed interaction evaluated, as the reference kernel does
                              (default: the body system owns a workspace and every PAIR of bodies is evaluated once)
  --workspace-mib UINT        Spend at most this many MiB on that workspace (the pair tournament is then cut into slices that share
                              one region of reaction planes; default: what the library asks for, at most a third of the device's memory)
  --energy                    With --benchmark or --steps: print the kinetic, potential and total energy and the momentum before and
                              after the run, and the relative drift of the total energy (one device only)
  --energies                  With --systems (required; every --integrator=*-ensemble too) and --benchmark, --steps or --t-end: measure the
                              energy of every system at the start and at the end, in one call each (outside --benchmark's timed
                              region; the block ensembles are synchronised first), and print the smallest, median and largest total
                              energy at the start and, at the end, the system whose total drifted most, the largest and the rms
                              relative drift, the largest momentum drift and the systems whose drift is not finite
  --neighbours FLOAT          After a --benchmark, --steps or --dump run: print the closest pair of bodies and its separation, the mean and
                              the largest number of neighbours within this radius (>= 0) and its body, the deepest potential and its
                              body (one device only, at most 16777216 bodies; accepted wherever --energy is)
  --knn UINT                  After a --benchmark, --steps or --dump run: from the K (2 to 16) nearest neighbours of every body print the
                              density centre, the density and core radii, the densest body, the smallest and largest K-th-neighbour
                              distance and the 10 %, 50 % and 90 % Lagrangian radii about the density centre (one device only, at
                              most 16777216 bodies; accepted wherever --neighbours is)
  --field FILE                After a --benchmark, --steps or --dump run: print the acceleration and the potential of the final state at
                              every point of this text file (one `x y z` per line, `#` comments, 1 to 65536 points; softened as the
                              run, no body excluded; one device only; accepted wherever --energy is)
  --inject-error FLOAT        Test hook: added to body 0's x of the fast result before --compare checks it
  --systems UINT              Step this many independent systems of --numbodies (<= 65536, required) bodies in one launch: system 0
                              is the single-system start-up state, the others the next draws; --benchmark counts B*N^2 interactions
                              per step, --dump writes every system's positions, then every system's velocities
  --integrator TEXT [euler]   euler | hermite | hermite-block.  hermite: 4th-order Hermite predictor-corrector steps (acceleration and
                              jerk per interaction, no damping) of --numbodies (required) bodies on one device, FAST arithmetic; with
                              --benchmark, --steps, --dump and --energy.  hermite-block: the same scheme with block time steps: every
                              body steps by its own dt * 2^-level, --steps=K advances to K * dt, interactions are counted as n_act * N
  --eta FLOAT [0.02]          hermite-block: accuracy parameter of the bodies' time steps (the first steps use 0.01)
  --levels UINT [30]          hermite-block: the deepest level, 0 to 40 (time steps down to dt * 2^-levels)
  --integrator=hermite6       hermite's run and restrictions with the 6th-order scheme: acceleration, jerk and snap per interaction, the
                              global error falls with dt^6
  --integrator=hermite6-block  hermite-block's run, restrictions, --eta and --levels with the 6th-order scheme.  --eta [0.2]: it sits
                              inside the root of the step criterion as in hermite-block, and 0.2 here does what 0.02 does there, with a
                              quarter of the block steps
  --integrator=hermite-ensemble  with --systems (required; its restrictions apply, numbodies * systems at most 2^28): Hermite steps of every
                              system in one launch per stage.  --steps=K takes K steps of --integrator=hermite's dt, --dump writes in
                              --systems' format, --benchmark counts B*N^2 acceleration + jerk interactions per step
  --t-end FLOAT               hermite-ensemble: run every system to this time (> 0) with a time step of its own, eta (--eta) times the
                              smallest |a| / |jerk| of the system, and print the systems done and stalled and the fewest, median and
                              most steps per system
  --integrator=hermite-block-ensemble  with --systems (required; its restrictions apply, numbodies * systems at most 2^28): block time steps
                              (hermite-block's scheme, --eta and --levels) of every system in the launches of one call, every system
                              with its own time.  --t-end=T (or --steps=K: T = K * dt) runs every system to its last block step not
                              past T; --dump writes every system synchronised at its own time, in --systems' format; --benchmark
                              times intervals of dt and counts the sum of n_act * N over the systems
  --integrator=hermite6-block-ensemble  hermite-block-ensemble's run, restrictions, --t-end, --steps, --dump and --benchmark with
                              hermite6-block's 6th-order scheme and its --eta [0.2]; the integrator is named hermite6-block in the
                              output.  dt and dt * 2^-levels must have normal cubes in the run's precision (single: --levels up to 36
                              with dt 0.016, up to 31 with --demo=2's dt 0.0006)
  --integrator=hermite6-ensemble  hermite-ensemble's run, restrictions, --steps, --t-end, --dump and --benchmark with the 6th-order scheme
                              (acceleration, jerk and snap per interaction).  --eta [0.025]: a system's time step is eta times the ROOT
                              of the smallest (|a||s| + |j|^2) / (|j||c| + |s|^2) of the system, so eta sits outside the root here;
                              0.025 ends a cloud with a hard binary with a thirtieth of the energy error of hermite-ensemble's 0.02
                              in four fifths of its steps, in --fp64; single-precision --t-end runs want --eta=0.2 or more (the
                              crackle of the step criterion is rounding noise below that, and systems stall)
  --alloc-limit-mib UINT      Test hook (needs LD_PRELOAD=libnbody_hip_lab.so): device allocations above this many MiB are refused
)";

template <typename I> auto parse_number(std::string_view text, I& out) -> bool {
    const auto* first = text.data();
    const auto* last  = text.data() + text.size();
    const auto [ptr, ec] = std::from_chars(first, last, out);
    return ec == std::errc{} && ptr == last;
}

auto parse_args(int argc, char** argv) -> std::pair<Status, Options> {
    auto options = Options{};

    auto error = [&](const std::string& message) {
        std::fprintf(stderr,
                     "-------------------------------------------\n"
                     "CRITICAL ERROR:\n"
                     "%s\n"
                     "-------------------------------------------\n\n",
                     message.c_str());
        std::fprintf(stderr, "%s\n", help_text);
        return std::pair(Status::InvalidArguments, options);
    };

    for (int a = 1; a < argc; ++a) {
        auto arg = std::string_view(argv[a]);
        if (arg == "-h" || arg == "--help" || arg == "-help") {
            std::printf("%s\n", help_text);
            return std::pair(Status::CleanShutDown, options);
        }
        if (arg.size() < 2 || arg[0] != '-') return error("The following argument was not expected: " + std::string(arg));
        // "-name" and "--name" are the same option (the NVIDIA sample used one dash, CLI11 in the reference two)
        auto name = arg.substr(arg[1] == '-' ? 2 : 1);
        std::optional<std::string_view> value;
        if (const auto eq = name.find('='); eq != std::string_view::npos) {
            value = name.substr(eq + 1);
            name  = name.substr(0, eq);
        }
        auto take_value = [&]() -> std::optional<std::string_view> {
            if (value) return value;
            if (a + 1 < argc) return std::string_view(argv[++a]);
            return std::nullopt;
        };
        auto flag = [&](bool& target) -> bool {
            if (value) return false;
            target = true;
            return true;
        };

        bool ok = true;
        if (name == "fullscreen") ok = flag(options.fullscreen);
        else if (name == "fp64") ok = flag(options.fp64);
        else if (name == "hostmem") ok = flag(options.hostmem);
        else if (name == "benchmark") ok = flag(options.benchmark);
        else if (name == "compare") ok = flag(options.compare);
        else if (name == "qatest") ok = flag(options.qatest);
        else if (name == "cpu") ok = flag(options.cpu);
        else if (name == "graph") ok = flag(options.graph);
        else if (name == "no-workspace" || name == "no_workspace") ok = flag(options.no_workspace);
        else if (name == "energy") ok = flag(options.energy);
        else if (name == "energies") ok = flag(options.energies);
        else if (name == "numbodies") {
            const auto v = take_value();
            ok           = v && parse_number(*v, options.numbodies) && options.numbodies >= 1;
            if (!ok) return error("--numbodies: Value not in range 1 to " + std::to_string(std::numeric_limits<std::size_t>::max()));
        } else if (name == "i" || name == "iterations") {
            const auto v = take_value();
            ok           = v && parse_number(*v, options.iterations);
        } else if (name == "blockSize") {
            const auto v = take_value();
            ok           = v && parse_number(*v, options.block_size);
        } else if (name == "systems") {
            const auto v = take_value();
            ok           = v && parse_number(*v, options.systems) && options.systems >= 1 && options.systems <= 0xFFFFFFFFu;
            if (!ok) return error("--systems: Value not in range 1 to 4294967295");
        } else if (name == "steps") {
            const auto v = take_value();
            ok           = v && parse_number(*v, options.steps);
        } else if (name == "workspace-mib" || name == "workspace_mib") {
            const auto v = take_value();
            ok           = v && parse_number(*v, options.workspace_mib);
        } else if (name == "alloc-limit-mib") {
            const auto v = take_value();
            ok           = v && parse_number(*v, options.alloc_limit_mib);
        } else if (name == "seed") {
            const auto v = take_value();
            unsigned   s = 0;
            ok           = v && parse_number(*v, s);
            if (ok) options.seed = s;
        } else if (name == "tipsy") {
            const auto v = take_value();
            ok           = v.has_value();
            if (ok) {
                options.tipsy = std::filesystem::path(std::string(*v));
                if (!std::filesystem::is_regular_file(options.tipsy)) return error("--tipsy: File does not exist: " + options.tipsy.string());
            }
        } else if (name == "dump") {
            const auto v = take_value();
            ok           = v.has_value();
            if (ok) options.dump = std::filesystem::path(std::string(*v));
        } else if (name == "numdevices") {
            const auto v = take_value();
            int        n = 0;
            ok           = v && parse_number(*v, n) && n >= 1;
            if (!ok) return error("--numdevices: Value not in range 1 to " + std::to_string(std::numeric_limits<int>::max()));
            options.devices.clear();
            for (int d = 0; d < n; ++d) options.devices.push_back(d);
        } else if (name == "devices") {
            const auto v = take_value();
            ok           = v.has_value() && !v->empty();
            options.devices.clear();
            auto rest = ok ? *v : std::string_view{};
            while (ok && !rest.empty()) {
                const auto comma = rest.find(',');
                int        d     = -1;
                ok               = parse_number(rest.substr(0, comma), d) && d >= 0;
                options.devices.push_back(d);
                rest = comma == std::string_view::npos ? std::string_view{} : rest.substr(comma + 1);
            }
        } else if (name == "demo") {
            const auto  v = take_value();
            std::size_t d = 0;
            ok            = v && parse_number(*v, d) && d < Compute::demo_params.size();
            if (!ok) return error("--demo: Value not in range 0 to " + std::to_string(Compute::demo_params.size() - 1));
            options.demo = d;
        } else if (name == "inject-error") {
            const auto v = take_value();
            ok           = v.has_value();
            if (ok) {
                char* end            = nullptr;
                const auto text      = std::string(*v);
                options.inject_error = std::strtod(text.c_str(), &end);
                ok                   = end != nullptr && *end == '\0' && end != text.c_str();
            }
        } else if (name == "mode") {
            const auto v = take_value();
            ok           = v && (*v == "fast" || *v == "strict");
            if (ok) options.mode = (*v == "strict") ? NB_MODE_STRICT : NB_MODE_FAST;
        } else if (name == "integrator") {
            const auto v = take_value();
            ok           = v && (*v == "euler" || *v == "hermite" || *v == "hermite6" || *v == "hermite-block" || *v == "hermite6-block" || *v == "hermite-ensemble" || *v == "hermite-block-ensemble" ||
                            *v == "hermite6-ensemble" || *v == "hermite6-block-ensemble");
            if (ok) {
                options.hermite6_ensemble = *v == "hermite6-ensemble";
                options.hermite_ensemble = *v == "hermite-ensemble" || options.hermite6_ensemble, options.hermite6_block_ensemble = *v == "hermite6-block-ensemble";
                options.hermite_block_ensemble = *v == "hermite-block-ensemble" || options.hermite6_block_ensemble;
                options.hermite6_block = *v == "hermite6-block";
                options.hermite = (*v == "hermite" || *v == "hermite6" || *v == "hermite-block" || options.hermite6_block);
                options.hermite_block = (*v == "hermite-block" || options.hermite6_block), options.hermite6 = *v == "hermite6";
            }
        } else if (name == "eta") {
            const auto v = take_value();
            ok           = v.has_value();
            if (ok) {
                char*      end  = nullptr;
                const auto text = std::string(*v);
                const auto eta  = std::strtod(text.c_str(), &end);
                ok              = end != nullptr && *end == '\0' && end != text.c_str() && eta > 0.0 && eta <= 1.0;
                if (!ok) return error("--eta: Value not in range (0, 1]");
                options.eta = eta;
            }
        } else if (name == "t-end") {
            const auto v = take_value();
            ok           = v.has_value();
            if (ok) {
                char*      end   = nullptr;
                const auto text  = std::string(*v);
                const auto t_end = std::strtod(text.c_str(), &end);
                ok               = end != nullptr && *end == '\0' && end != text.c_str() && std::isfinite(t_end) && t_end > 0.0;
                if (!ok) return error("--t-end: Value not a time (a finite number > 0)");
                options.t_end = t_end;
            }
        } else if (name == "neighbours") {
            const auto v = take_value();
            ok           = v.has_value();
            if (ok) {
                char*      end    = nullptr;
                const auto text   = std::string(*v);
                const auto radius = std::strtod(text.c_str(), &end);
                ok                = end != nullptr && *end == '\0' && end != text.c_str() && std::isfinite(radius) && radius >= 0.0;
                if (!ok) return error("--neighbours: Value not a radius (a finite number >= 0)");
                options.neighbours = radius;
            }
        } else if (name == "knn") {
            const auto v = take_value();
            unsigned   k = 0;
            ok           = v && parse_number(*v, k) && k >= 2 && k <= NB_KNN_MAX_K;
            if (!ok) return error("--knn: Value not in range 2 to 16");
            options.knn = k;
        } else if (name == "field") {
            const auto v = take_value();
            ok           = v.has_value();
            if (ok) {
                if (const auto message = read_field_points(std::filesystem::path(std::string(*v)), options.field_points); !message.empty()) return error(message);
            }
        } else if (name == "levels") {
            const auto v = take_value();
            int        l = 0;
            ok           = v && parse_number(*v, l) && l >= 0 && l <= NB_HERMITE_BLOCK_MAX_LEVEL;
            if (!ok) return error("--levels: Value not in range 0 to 40");
            options.levels = l;
        } else if (name == "config") {
            const auto v = take_value();
            ok           = v && (*v == "shell" || *v == "random" || *v == "expand");
            if (ok) options.config = *v == "shell" ? NBodyConfig::NBODY_CONFIG_SHELL : *v == "random" ? NBodyConfig::NBODY_CONFIG_RANDOM : NBodyConfig::NBODY_CONFIG_EXPAND;
        } else {
            return error("The following argument was not expected: " + std::string(arg));
        }
        if (!ok) return error("Could not parse argument: " + std::string(arg));
    }

    // combinations judged once every argument is in (--numdevices may come after --energy)
    if (options.energy && options.devices.size() > 1) return error("--energy is single-device: it cannot be combined with --numdevices or --devices naming more than one GPU");
    if (options.energy && (options.compare || options.qatest)) return error("--energy cannot be combined with --compare or --qatest (those runs step two systems)");

    if (options.energies && options.systems == 0) return error("--energies measures every system of a --systems run: it needs --systems (one system: --energy)");

    if (options.neighbours && options.devices.size() > 1) return error("--neighbours is single-device: it cannot be combined with --numdevices or --devices naming more than one GPU");
    if (options.neighbours && (options.compare || options.qatest)) return error("--neighbours cannot be combined with --compare or --qatest (those runs step two systems)");
    if (options.neighbours && options.numbodies > NB_NEIGHBOUR_MAX_BODIES) return error("--neighbours: --numbodies must be at most 16777216");

    if (options.knn && options.devices.size() > 1) return error("--knn is single-device: it cannot be combined with --numdevices or --devices naming more than one GPU");
    if (options.knn && (options.compare || options.qatest)) return error("--knn cannot be combined with --compare or --qatest (those runs step two systems)");
    if (options.knn && options.numbodies > NB_NEIGHBOUR_MAX_BODIES) return error("--knn: --numbodies must be at most 16777216");

    const auto field = !options.field_points.empty();
    if (field && options.devices.size() > 1) return error("--field is single-device: it cannot be combined with --numdevices or --devices naming more than one GPU");
    if (field && (options.compare || options.qatest)) return error("--field cannot be combined with --compare or --qatest (those runs step two systems)");

    if (options.systems > 0) {
        if (options.numbodies == 0) return error("--systems needs an explicit --numbodies of at most 65536 (the single-system default, blockSize * 4 * CUs, is above the ensemble limit)");
        if (options.numbodies > 65536) return error("--systems: --numbodies must be at most 65536 (above that one system fills the GPU: run it without --systems)");
        if (options.numbodies * options.systems > (std::size_t{1} << 31)) return error("--systems: numbodies * systems must be at most 2^31");
        if (options.devices.size() > 1) return error("--systems is single-device: it cannot be combined with --numdevices or --devices naming more than one GPU");
        if (options.hostmem || !options.tipsy.empty() || options.compare || options.qatest || options.graph || options.energy || options.neighbours || options.knn || field || options.no_workspace || options.workspace_mib != 0 || options.cpu) {
            return error("--systems cannot be combined with --hostmem, --tipsy, --compare, --qatest, --graph, --energy, --neighbours, --knn, --field, --no-workspace, --workspace-mib or --cpu");
        }
    }

    if (options.hermite) {
        if (options.numbodies == 0) return error("--integrator=hermite needs an explicit --numbodies");
        if (options.numbodies > NB_HERMITE_MAX_BODIES) return error("--integrator=hermite: --numbodies must be at most 67108864");
        if (options.hermite_block && options.numbodies > NB_HERMITE_BLOCK_MAX_BODIES) return error("--integrator=hermite-block: --numbodies must be at most 16777216");
        if (options.mode == NB_MODE_STRICT) return error("--integrator=hermite has no strict mode: there is no CPU reference arithmetic to reproduce");
        if (options.devices.size() > 1) return error("--integrator=hermite is single-device: it cannot be combined with --numdevices or --devices naming more than one GPU");
        if (options.systems > 0) return error("--integrator=hermite cannot be combined with --systems");
        if (options.hostmem || !options.tipsy.empty() || options.compare || options.qatest || options.graph || options.no_workspace || options.workspace_mib != 0 || options.cpu) {
            return error("--integrator=hermite cannot be combined with --hostmem, --tipsy, --compare, --qatest, --graph, --no-workspace, --workspace-mib or --cpu");
        }
    }

    if (options.hermite_ensemble) {
        if (options.systems == 0) return error("--integrator=hermite-ensemble needs --systems (and an explicit --numbodies of at most 65536)");
        if (options.numbodies * options.systems > NB_HERMITE_ENSEMBLE_MAX_TOTAL) return error("--integrator=hermite-ensemble: numbodies * systems must be at most 2^28");
        if (options.mode == NB_MODE_STRICT) return error("--integrator=hermite-ensemble has no strict mode: there is no CPU reference arithmetic to reproduce");
        if (options.t_end && (options.benchmark || options.steps > 0)) return error("--t-end cannot be combined with --benchmark or --steps (it runs every system to that time)");
    }
    if (options.hermite_block_ensemble) {
        if (options.systems == 0) return error("--integrator=hermite-block-ensemble needs --systems (and an explicit --numbodies of at most 65536)");
        if (options.numbodies * options.systems > NB_HERMITE_BLOCK_ENSEMBLE_MAX_TOTAL) return error("--integrator=hermite-block-ensemble: numbodies * systems must be at most 2^28");
        if (options.mode == NB_MODE_STRICT) return error("--integrator=hermite-block-ensemble has no strict mode: there is no CPU reference arithmetic to reproduce");
        if (options.t_end && (options.benchmark || options.steps > 0)) return error("--t-end cannot be combined with --benchmark or --steps (it runs every system to that time)");
    }
    if (options.hermite6_block_ensemble) {
        // the "Range of h" of nbody_hip_hermite6_block.h: the corrector divides by the cube of a step, formed in the run's precision
        const double dt_max = static_cast<double>(Compute::demo_params[options.demo.value_or(0)].time_step);
        const auto   cube_is_normal = [&](double step) {
            if (options.fp64) return std::isnormal(step * step * step);
            const float h = static_cast<float>(step), hh = h * h;
            return std::isnormal(hh * h);
        };
        if (!cube_is_normal(dt_max) || !cube_is_normal(std::ldexp(dt_max, -options.levels.value_or(30)))) {
            return error("--integrator=hermite6-block-ensemble: dt * 2^-levels must have a normal cube in the run's precision (fewer --levels, or --fp64)");
        }
    }
    if (options.t_end && !options.hermite_ensemble && !options.hermite_block_ensemble) return error("--t-end belongs to --integrator=hermite-ensemble");

    // (--eta is hermite-ensemble's too, and both are hermite-block-ensemble's; the message is the one the block integrator's users know)
    if ((options.levels && !options.hermite_block && !options.hermite_block_ensemble) || (options.eta && !options.hermite_block && !options.hermite_ensemble && !options.hermite_block_ensemble)) {
        return error("--eta and --levels belong to --integrator=hermite-block");
    }

    // the reference prints this hint and the full help on every successful parse (nbody.cpp:315-316)
    std::printf("Run \" nbody - benchmark[-numbodies = <numBodies>] \" to measure performance\n");
    std::printf("%s\n", help_text);
    return std::pair(Status::OK, options);
}

auto print_energy(const char* what, const nb_energy_t& e) -> void {
    std::printf("%s: kinetic=%.9g potential=%.9g total=%.9g momentum=%.9g,%.9g,%.9g", what, e.kinetic, e.potential, e.total, e.momentum[0], e.momentum[1], e.momentum[2]);
}

template <typename T> auto dump_state(const std::filesystem::path& file, std::span<const T> pos, std::span<const T> vel) -> void {
    auto out = std::ofstream(file, std::ios::binary | std::ios::trunc);
    if (!out) throw std::runtime_error("cannot open dump file " + file.string());
    out.write(reinterpret_cast<const char*>(pos.data()), static_cast<std::streamsize>(pos.size_bytes()));
    out.write(reinterpret_cast<const char*>(vel.data()), static_cast<std::streamsize>(vel.size_bytes()));
}

}  // namespace

auto main(int argc, char** argv) -> int {
    try {
        const auto [status, cmd_options] = parse_args(argc, argv);
        if (Status::InvalidArguments == status) return 1;
        if (Status::CleanShutDown == status) return 0;

        std::printf("NOTE: The HIP N-body hot path.  Results may vary with the GPU's power state.\n\n");
        std::printf("> %s mode\n", cmd_options.fullscreen ? "Fullscreen" : "Windowed");

        if (cmd_options.seed) std::srand(*cmd_options.seed);
        nbody_hip::integration_mode() = cmd_options.mode;
        nbody_hip::use_workspace()    = !cmd_options.no_workspace;
        nbody_hip::workspace_cap_bytes() = cmd_options.workspace_mib << 20;
        if (cmd_options.alloc_limit_mib != 0) {
            // nb_set_alloc_limit is exported by libnbody_hip_lab.so only (include/nbody_hip_lab.h): the tests preload that library
            using SetLimit   = int (*)(std::size_t);
            const auto limit = reinterpret_cast<SetLimit>(dlsym(RTLD_DEFAULT, "nb_set_alloc_limit"));
            if (limit == nullptr) throw std::invalid_argument("--alloc-limit-mib is a test hook of the lab library: run with LD_PRELOAD=libnbody_hip_lab.so");
            (void)limit(cmd_options.alloc_limit_mib << 20);
        }

        if (cmd_options.systems > 0) {
            if (!cmd_options.benchmark && cmd_options.steps == 0 && cmd_options.dump.empty() && !cmd_options.t_end) throw std::invalid_argument("--systems: pass --benchmark or --steps/--dump");
            auto run        = EnsembleRun{};
            run.fp64        = cmd_options.fp64;
            run.num_bodies  = cmd_options.numbodies;
            run.num_systems = cmd_options.systems;
            run.mode        = cmd_options.mode;
            run.config      = cmd_options.config;
            run.params      = Compute::demo_params[cmd_options.demo.value_or(0)];
            run.benchmark   = cmd_options.benchmark;
            run.iterations  = cmd_options.iterations == 0 ? 10 : static_cast<int>(cmd_options.iterations);
            run.steps       = cmd_options.steps;
            run.dump        = cmd_options.dump;
            run.hermite     = cmd_options.hermite_ensemble;
            run.t_end       = cmd_options.t_end.value_or(0.0);
            run.sixth       = cmd_options.hermite6_ensemble || cmd_options.hermite6_block_ensemble;
            run.eta         = cmd_options.eta.value_or(cmd_options.hermite6_ensemble ? kHermite6EnsembleEta : cmd_options.hermite6_block_ensemble ? 0.2 : run.eta);
            run.block       = cmd_options.hermite_block_ensemble;
            run.levels      = cmd_options.levels.value_or(run.levels);
            run.energies    = cmd_options.energies;
            run_ensemble(run);
            return 0;
        }

        if (cmd_options.hermite) {
            if (!cmd_options.benchmark && cmd_options.steps == 0 && cmd_options.dump.empty()) throw std::invalid_argument("--integrator=hermite: pass --benchmark or --steps/--dump");
            auto run       = HermiteRun{};
            run.fp64       = cmd_options.fp64;
            run.num_bodies = cmd_options.numbodies;
            run.config     = cmd_options.config;
            run.params     = Compute::demo_params[cmd_options.demo.value_or(0)];
            run.benchmark  = cmd_options.benchmark;
            run.iterations = cmd_options.iterations == 0 ? 10 : static_cast<int>(cmd_options.iterations);
            run.steps      = cmd_options.steps;
            run.dump       = cmd_options.dump;
            run.energy     = cmd_options.energy;
            run.neighbours = cmd_options.neighbours.value_or(-1.0);
            run.knn        = cmd_options.knn.value_or(0u);
            run.field_points = cmd_options.field_points;
            run.block      = cmd_options.hermite_block;
            run.sixth      = cmd_options.hermite6 || cmd_options.hermite6_block;
            run.eta        = cmd_options.eta.value_or(cmd_options.hermite6_block ? 0.2 : run.eta);
            run.levels     = cmd_options.levels.value_or(run.levels);
            run_hermite(run);
            return 0;
        }

        const auto compare_to_cpu = (cmd_options.compare || cmd_options.qatest) && (!cmd_options.cpu);
        const auto headless_run   = cmd_options.benchmark || compare_to_cpu || cmd_options.steps > 0 || !cmd_options.dump.empty();
        if (!headless_run && !cmd_options.cpu) {
            throw std::invalid_argument("the interactive OpenGL viewer is out of scope on a headless accelerator: pass --benchmark, --compare/--qatest or --steps/--dump");
        }

        auto compute = Compute(cmd_options.fp64, cmd_options.cpu, compare_to_cpu, cmd_options.benchmark, cmd_options.hostmem, cmd_options.block_size, cmd_options.numbodies, cmd_options.tipsy, cmd_options.config, cmd_options.devices);

        compute.use_graph(cmd_options.graph);
        if (cmd_options.demo) compute.select_demo(*cmd_options.demo);
        const auto measure_energy = cmd_options.energy && (cmd_options.benchmark || cmd_options.steps > 0);
        const auto energy_start   = measure_energy ? std::optional<nb_energy_t>(compute.energy()) : std::nullopt;
        // after the run's own output: the energy at the start and at the end, and how far the total drifted over `steps` steps
        const auto report_energy = [&](std::size_t steps) {
            if (!energy_start) return;
            const auto end = compute.energy();
            print_energy("energy start", *energy_start);
            std::printf("\n");
            const auto label = "energy end (" + std::to_string(steps) + " steps)";
            print_energy(label.c_str(), end);
            std::printf(" relative_drift=%.9g\n", (end.total - energy_start->total) / std::abs(energy_start->total));
        };
        // ... and then the neighbourhood of the final state (softened as the run)
        const auto report_neighbourhood = [&]() {
            if (!cmd_options.neighbours) return;
            const auto softening = compute.active_params().softening;
            if (compute.fp64_enabled()) {
                report_neighbours(compute.positions_fp64(), *cmd_options.neighbours, static_cast<double>(softening) * static_cast<double>(softening));
            } else {
                report_neighbours(compute.positions_fp32(), *cmd_options.neighbours, softening * softening);
            }
        };
        // ... and then its density centre and radii
        const auto report_structure = [&]() {
            if (!cmd_options.knn) return;
            if (compute.fp64_enabled()) {
                report_knn(compute.positions_fp64(), *cmd_options.knn);
            } else {
                report_knn(compute.positions_fp32(), *cmd_options.knn);
            }
        };
        // ... and then its field at the points of --field
        const auto report_field_points = [&]() {
            if (cmd_options.field_points.empty()) return;
            const auto softening = compute.active_params().softening;
            if (compute.fp64_enabled()) {
                report_field(compute.positions_fp64(), cmd_options.field_points, static_cast<double>(softening) * static_cast<double>(softening));
            } else {
                report_field(compute.positions_fp32(), cmd_options.field_points, softening * softening);
            }
        };
        if (cmd_options.benchmark) {
            const auto nb_iterations = cmd_options.iterations == 0 ? 10 : static_cast<int>(cmd_options.iterations);
            compute.run_benchmark(nb_iterations);
            report_energy(1 + static_cast<std::size_t>(nb_iterations));  // (run_benchmark takes one untimed step first)
            report_neighbourhood();
            report_structure();
            report_field_points();
            return 0;
        }
        if (compare_to_cpu) {
            if (cmd_options.steps > 0) compute.report_trajectory_error(cmd_options.steps);  // (before the check steps the system)
            const auto result = compute.compare_results(cmd_options.inject_error);
            return static_cast<int>(!result);
        }
        for (auto s = std::size_t{0}; s < cmd_options.steps; ++s) compute.update_simulation();
        if (!cmd_options.dump.empty()) {
            if (compute.fp64_enabled()) {
                dump_state<double>(cmd_options.dump, compute.positions_fp64(), compute.velocities_fp64());
            } else {
                dump_state<float>(cmd_options.dump, compute.positions_fp32(), compute.velocities_fp32());
            }
        }
        report_energy(cmd_options.steps);
        report_neighbourhood();
        report_structure();
        report_field_points();
        return 0;
    } catch (const std::invalid_argument& e) {
        std::fprintf(stderr, "ERROR: %s\n", e.what());
        return 1;
    } catch (const std::bad_alloc&) {
        std::fprintf(stderr, "ERROR: Unable to allocate memory!\n");
        return 3;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "ERROR: %s\n", e.what());
        return 2;
    } catch (...) {
        std::printf("ERROR: An unknown error occurred! Please inform your local developer!\n");
        return 4;
    }
}
