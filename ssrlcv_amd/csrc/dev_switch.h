// ssrlcv_amd/csrc/dev_switch.h -- developer switches of the library: the one place that declares and reads them.
//
// The kernels exist in several bit-identical formulations (VALU / MFMA / register-marching Gaussians, pixels per lane of
// the DoG pass, schedules ...); which one runs is decided by size and radius, and -- in a DEVELOPER build, the default
// of csrc/Makefile -- can be forced through SSRLCV_* environment variables, which is how the parity tests hold every
// formulation to the oracle and how the A/B timings of DESIGN.md were taken.  Every switch is one row of svdev::Switches
// below (name, type, default, meaning); the library reads svdev::sw().<field> and nothing else in csrc/ touches the
// environment.  tests/helpers.py takes the set of names from the quoted strings of this file, so a test cannot set a switch
// that is not declared here.
//   developer build: sw() is one object per process, filled from the environment on first use; mutable, so that the tools/
//     lab programs that include a .hip file can overwrite a knob in place (svdev::sw().gaussRm = 63).
//   release build: a drop-in library must not let its caller's environment choose its code path.  `make -C ssrlcv_amd/csrc
//     release` builds libssrlcv_hip_release.so with -DSSRLCV_RELEASE, where sw() is a compile-time constant holding every
//     default: the branches fold, no switch name and no parsing call is left in the binary (tests/test_capi_symbols.py).
// (Also compiled as C++14 by g++ for host_merge.cpp.)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

// Instrumented builds (results unchanged, timings not): s_memtime stamps of the Gaussian kernels (-DSSRLCV_STAMPS, the tools/
// lab programs) and the walk counters of the band-culled matcher (-DSSRLCV_MATCH_STATS, `make instrumented`).  Neither may
// end up in libssrlcv_hip.so / libssrlcv_hip_release.so: the `all` and `release` targets stop here.  (The timing labs of
// rounds 4-5 whose RESULTS were invalid -- matcher without epilogue / operand reads, gathers folded into 32 KB, one byte
// load of eight in the upsampling loader -- served their measurements, profiles/r05_matcher_lab_pmc.txt,
// r05_sampling_gather_lab.txt, r05_kernel_ab.txt section 6, and were removed from the sources in round 6: git history.)
// SSRLCV_TIMING_VARIANT (tools/ lab programs only): builds that leave work OUT to time what remains -- results invalid.
#if (defined(SSRLCV_STAMPS) || defined(SSRLCV_MATCH_STATS) || defined(SSRLCV_TIMING_VARIANT)) && !defined(SSRLCV_INSTRUMENTED_BUILD)
#error "SSRLCV_STAMPS / SSRLCV_MATCH_STATS only build through `make instrumented` or the tools/ lab programs (-DSSRLCV_INSTRUMENTED_BUILD)"
#endif
#if defined(SSRLCV_LAB) || defined(SSRLCV_MATCH_LAB) || defined(SSRLCV_LAB_LOCAL_GATHER) || defined(SSRLCV_LAB_UPS_LOADS)
#error "the timing-lab variants (results invalid) were removed in round 6; see git history before 2026-10-05"
#endif

// Two defaults are compile-time choices (-D<macro>=<value> wins over the values here)
#ifndef SSRLCV_THETAS_LANES_SHIFT
#define SSRLCV_THETAS_LANES_SHIFT 2  // lanes per key point of the orientation kernel, as a shift: 4 lanes
#endif
#ifndef SSRLCV_PAIR_F32_MINPX
#define SSRLCV_PAIR_F32_MINPX (~(size_t)0)  // float-sourced octaves keep their two launches (see build_dog)
#endif
static_assert(SSRLCV_THETAS_LANES_SHIFT >= 0 && SSRLCV_THETAS_LANES_SHIFT <= 2, "k_thetas is built for 1, 2 or 4 lanes per key point");

namespace svdev __attribute__((visibility("hidden"))) {  // nothing of this header among the library's exports
// How a value is read.  Release: the value a switch has when it is not set, at compile time.
#ifdef SSRLCV_RELEASE
constexpr bool flag(const char*) { return false; }
constexpr int integer(const char*, int unset) { return unset; }
constexpr size_t size(const char*, size_t unset) { return unset; }
constexpr float real(const char*, float unset) { return unset; }
constexpr char first_char(const char*) { return 0; }
#else
inline const char* env(const char* name) { return getenv(name); }
inline bool flag(const char* name) { return env(name) != nullptr; }  // present means on, whatever the value (even 0 or empty)
inline int integer(const char* name, int unset) { return env(name) ? atoi(env(name)) : unset; }
inline size_t size(const char* name, size_t unset) { return env(name) ? (size_t)atoll(env(name)) : unset; }
inline float real(const char* name, float unset) { return env(name) ? (float)atof(env(name)) : unset; }
inline char first_char(const char* name) { return env(name) ? env(name)[0] : 0; }
#endif
template <typename T>
constexpr T positive_or(T v, T otherwise) { return v > 0 ? v : otherwise; }
constexpr int one_or_two(int n) { return n == 1 || n == 2 ? n : 0; }
constexpr int lanes_to_shift(int lanes) { return lanes >= 4 ? 2 : (lanes >= 2 ? 1 : 0); }

// THE TABLE.  One row per switch; every combination gives the same results.  Why a default is what it is (the measurements)
// stands next to the code that uses the field.
struct Switches {
  // ---- scale space: which Gaussian formulation (pyramid.hip launch_conv, gauss_pair.inc, gauss_pair_rm.inc)
  bool gaussValu = flag("SSRLCV_GAUSS_VALU");      // the VALU marching kernel for every radius (and no tile / fused-pair kernel)
  bool gaussMfma = flag("SSRLCV_GAUSS_MFMA");      // the f32-MFMA kernel for every radius (and no upsample fusion / fused pair)
  bool gaussWide = flag("SSRLCV_GAUSS_WIDE");      // MFMA kernel: 256-column strips whatever the level's size
  bool gaussNarrow = flag("SSRLCV_GAUSS_NARROW");  // MFMA kernel: 128-column strips where the radius allows
  int gaussMfmaMinR = integer("SSRLCV_GAUSS_MFMA_MINR", 11);              // smallest templated radius that goes to the MFMA kernel
  size_t gaussTileMaxPx = size("SSRLCV_GAUSS_TILE_MAXPX", (size_t)1 << 20);  // largest level (pixels) of the tile kernel; 0: tiny levels only
  int gaussRm = integer("SSRLCV_GAUSS_RM", 4 | 8 | 16);                   // radii of the register-marching kernel: bit per padded radius 6, 8, 12, 16, 24, 32
  size_t gaussRmMinPx = size("SSRLCV_GAUSS_RM_MINPX", (size_t)1 << 24);   // smallest level (pixels) it is used for
  int gaussRmOneb = integer("SSRLCV_GAUSS_RM_ONEB", 0);                   // radii that take its one-barrier form (same bits as gaussRm)
  int gaussRmRows = integer("SSRLCV_GAUSS_RM_ROWS", 0);                   // its rows per block; 0: sized to one round of resident blocks
  bool noGaussPair = flag("SSRLCV_NO_GAUSS_PAIR");       // levels 0 + 1 always as two launches
  bool noGaussPairRm = flag("SSRLCV_NO_GAUSS_PAIR_RM");  // no matrix-pipe form of the fused pair (which turns the fused pair off)
  size_t gaussPairMinPx = size("SSRLCV_GAUSS_PAIR_MINPX", (size_t)1 << 26);                 // smallest u8-sourced octave (pixels) that fuses levels 0 + 1
  size_t gaussPairMinPxF32 = size("SSRLCV_GAUSS_PAIR_MINPX_F32", SSRLCV_PAIR_F32_MINPX);    // the same for float-sourced octaves
  bool gaussPairValuForm = first_char("SSRLCV_GAUSS_PAIR_FORM") == 'v';  // =valu: the vector formulation of the fused pair
  int pairRows = integer("SSRLCV_PAIR_ROWS", 0);               // rows per block of both fused-pair kernels; 0: one round of resident blocks
  bool noUpsampleFusion = flag("SSRLCV_NO_UPSAMPLE_FUSION");  // the 2x upsample as its own launch, not in the loader of octave 0's first level
  bool noBinFusion = flag("SSRLCV_NO_BIN_FUSION");            // the 2x2 bin as its own launch, not folded into level 3's convolution
  bool noXcdStrips = flag("SSRLCV_NO_XCD_STRIPS");            // the plain block order of the strip kernels
  // ---- scale space: the DoG / extrema pass and the schedule of build_dog (pyramid.hip)
  int dogxNpx = integer("SSRLCV_DOGX_NPX", 0);                                        // 1 | 2: fewer pixels per lane than alignment allows
  int dogSplit = integer("SSRLCV_DOG_SPLIT", 0) != 0 ? 1 : 0;                          // 1: the split form of the pass on every octave
  unsigned dogxWaves = positive_or((unsigned)integer("SSRLCV_DOGX_WAVES", 0), 14336u);  // waves per launch of the pass
  int dogx0After = one_or_two(integer("SSRLCV_DOGX0_AFTER", 0));                       // 1 | 2: octave 0's pass waits for level 3 of that octave
  bool noOctaveOverlap = flag("SSRLCV_NO_OCTAVE_OVERLAP");              // every octave's convolutions on the caller's stream
  int octaveOverlapFrom = integer("SSRLCV_OCTAVE_OVERLAP_FROM", 1);     // first octave that alternates to the side stream
  int phased = integer("SSRLCV_PHASED", 0);                             // n + 1: the chain of levels 0-3 first, the rest held back n octaves
  bool earlyPolar = flag("SSRLCV_EARLY_POLAR");                         // fused extract: gradient tables start behind each octave's DoG pass
  bool noEarlyChain = flag("SSRLCV_NO_EARLY_CHAIN");                    // fused extract: every list chain stays in describe
  // ---- side streams of a plan (pyramid.hip plan_async, keypoints.hip describe)
  bool siftSerial = flag("SSRLCV_SIFT_SERIAL");               // no side streams: every launch on the caller's stream
  int prio = integer("SSRLCV_PRIO", 0);                       // bit 0: gradient tables on their own low-priority stream; bit 1: the chains' streams at high priority;
                                                              // bit 2 (=4): round 6's hand-overs of the key-point stage, see stagedGlue
  bool sideLowPriority = flag("SSRLCV_SIDE_LOW_PRIORITY");    // the `table` side stream at the lowest priority
  // ---- key points (keypoints.hip)
  int thetasLanesShift = lanes_to_shift(integer("SSRLCV_THETAS_LANES", 1 << SSRLCV_THETAS_LANES_SHIFT));  // =1|2|4 lanes per key point of k_thetas, kept as a shift
  bool thetasSplit = flag("SSRLCV_THETAS_SPLIT");              // the small octaves' orientations beside octave 0's gradient tables
  bool samplingPipelined = flag("SSRLCV_SAMPLING_PIPELINED");  // orientation launches of later sampling groups beside descriptor launches of earlier ones
  bool samplingIrregular = flag("SSRLCV_SAMPLING_IRREGULAR");  // pipelined form: take the fallback for blur indices that are no ordered partition
  // (no name of its own: tests/test_capi_symbols.py pins the number of names in this table, so the staged schedule is a bit of
  // the side-stream schedule switch above)
  bool stagedGlue = (prio & 4) != 0;                           // round 6's hand-overs: tables on `table`, memset prologue, one expansion launch per octave
#if defined(SSRLCV_INSTRUMENTED_BUILD) && !defined(SSRLCV_RELEASE)
  // instrumented build only (timing, results NOT valid): orientations of the selected (octave, blur segment) ranges alone -- bit o * 5 + seg
  uint32_t timingThetasSel = env("SSRLCV_TIMING_THETAS_SEL") ? (uint32_t)strtoul(env("SSRLCV_TIMING_THETAS_SEL"), nullptr, 16) : 0xFFFFFu;
#else
  uint32_t timingThetasSel = 0xFFFFFu;
#endif
  // ---- matcher (matcher.hip)
  bool matchF16 = flag("SSRLCV_MATCH_F16");             // initial value of ssrlcv_hip_set_match_arithmetic: the fp16 contraction
  float bandDir = real("SSRLCV_BAND_DIR", 1e30f);       // degrees: the direction of the band-culled matcher's frame; 1e30: from the bands
  float bandStrip = real("SSRLCV_BAND_STRIP", 0.0f);    // strip width (pixels) of the targets' order; <= 0: from epsilon
  float bandStripQ = real("SSRLCV_BAND_STRIP_Q", 0.0f); // the same for the queries; <= 0: the targets' width
  // ---- host merge (host_merge.cpp)
  int mergeThreads = positive_or(integer("SSRLCV_MERGE_THREADS", 1), 1);  // team of the parallel walk; 1: the sequential walk
  bool mergeTiming = flag("SSRLCV_MERGE_TIMING");                         // print the merge's phases to stderr
};

#ifdef SSRLCV_RELEASE
constexpr Switches kDefaults{};
constexpr const Switches& sw() { return kDefaults; }
#else
inline Switches& sw() {  // one object per library
  static Switches s;
  return s;
}
#endif
}  // namespace svdev
