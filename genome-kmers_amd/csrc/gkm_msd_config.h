// gkm_msd_config.h -- the MSD sort's tile, class and width constants, with their tuning overrides
// (GKM_PT, GKM_PI, GKM_WAVE_OCC8, GKM_WAVE_R8: tools/build_variant.sh).
// Private to gkm_msd.hip: every stage header (gkm_msd_*.h) and the host driver read these.
#pragma once

namespace gkm {

constexpr int kGR = 8;                  // global digit bits
constexpr int kGRadix = 1 << kGR;
// global partition tile: 1024 threads x 11 keys (tuning overrides GKM_PT / GKM_PI: tools/build_variant.sh)
#ifndef GKM_PT
#define GKM_PT 1024
#endif
#ifndef GKM_PI
#define GKM_PI 11
#endif
constexpr int kPT = GKM_PT, kPI = GKM_PI;
// wide L0 (msd0_wide_kernel): 11-bit digits over 18,432-position tiles of its own, 512 threads x 36
constexpr int kWideL0 = 11, kWT = 512, kWI = 36;
constexpr int kPTile = kPT * kPI;
constexpr int kChunkTiles = 256;        // tiles per scan chunk (GKM_TEST_CHUNK_TILES overrides: tests only)
constexpr int kBT = 512, kBI = 8, kBR = 8;    // block-local: 512 threads x 8 keys, 8-bit digit
constexpr int kBT2 = 1024, kBR2 = 10;         // big block-local: 1024 threads x 8 keys, 10-bit digit
                                              // (~5.9 K keys over 1024 digits: sub-buckets of ~6,
                                              // finished by rank-by-count, few re-listed)
constexpr int kBlockMax = kBT2 * kBI;   // 8192: larger buckets take another global level
// local finishing classes by bucket size: one wave x 4, 8 or 16 keys (msd_wave_kernel), 512
// threads x 8 keys (msd_local_kernel, <= 4096), 4 = tiny (<= kTiny elements: one thread per
// bucket), 5 = 1024 threads x 8 keys (<= 8192: the buckets an 11-bit L0 + one level leave at C3)
constexpr int kLocal = 6;
constexpr int kTiny = 8;
constexpr int kSmall = 24;                  // sub-buckets <= this: rank-by-count
// waves per SIMD the wave-local kernels' registers are capped for (msd_wave_kernel<I, W, .>); the
// LDS (7.2 KB per wave at I = 8) admits 5 per SIMD
#ifndef GKM_WAVE_OCC8
#define GKM_WAVE_OCC8 4
#endif
constexpr int kWaveOcc4 = 6, kWaveOcc8 = GKM_WAVE_OCC8, kWaveOcc16 = 3;
// digit bits of the wave-local kernels' in-LDS partition: buckets of ~370 keys (C3) over 512
// digits leave sub-buckets of ~0.7 keys (rank-by-count reads half of what 256 digits need)
#ifndef GKM_WAVE_R8
#define GKM_WAVE_R8 9
#endif
constexpr int kWaveR4 = 8, kWaveR8 = GKM_WAVE_R8, kWaveR16 = 10;
// later local rounds (buckets re-listed because a sub-bucket outgrew kSmall: repeat families) and
// later phases finish sub-buckets of up to kSmallLate by rank-by-count instead of re-listing them
// for another round -- a round costs a bucket load, ranking and write-back per bucket
constexpr int kSmallLate = 96;
// The local rounds write back the keys of a bucket only when some of its elements are re-listed
// (rare): the sort's product is the start order (+ group heads), and keys are re-encoded from the
// sorted starts when an API call needs them (gk_ctx::keys_stale).
constexpr int kMaxLevels = 16;              // global levels with a digit width of their own (wsched)

}  // namespace gkm
