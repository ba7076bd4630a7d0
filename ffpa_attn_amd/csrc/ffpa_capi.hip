// ffpa_capi.hip — the extern "C" boundary declared in include/ffpa_attn.h.
//
// Host-side argument validation mirrors what the reference checks in its launcher
// (csrc/cuffpa/launch.cuh:79-129: shapes, bias layout; ffpa_api.cc:193-197: dtype)
// but reports through status codes instead of TORCH_CHECK, allocates nothing and
// keeps no global mutable state beyond write-once per-device caches (the reference's process-global backend hint,
// csrc/cuffpa/backend.h:16-27, has no equivalent here: every choice is per call).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>

#include "ffpa_attn.h"
#include "ffpa_fwd_kernel.h"
#include "ffpa_fwd_m16_kernel.h"  // (FFPA_M16_MIN_D: the head dims whose prefill launches run the 16x16x32 build)
#include "ffpa_varlen_merge.h"   // (stage 2 of a KV-split packed-sequence launch)
#include "ffpa_launch.h"
#include "ffpa_paged.h"         // (the paged-KV twin of the packed-sequence kernel)
#include "ffpa_mla.h"           // (the MLA latent-cache kernels — the list of their variants, every variant's launcher — and the 16-bit appends)
#include "ffpa_mla_fp8.h"       // (the e4m3 variants' fourth argument struct and the quantising appends)
#include "ffpa_mla_sparse_ds.h"   // (the 656-byte FP8 rows of DeepSeek-V3.2: the row format, and the store that writes them)
#include "ffpa_mla_sparse_topk.h" // (the selection launch in front of the sparse latent calls)
#include "ffpa_kvcache_append.h"  // (the KV-cache append + rotary launch)
#include "ffpa_merge_states.h"    // (the merge of two attention states)
#include "ffpa_mla_cascade_plan.h"  // (the plan launch of a shared-prefix step over the MLA latent cache)

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

typedef int (*launch_fn)(int, int, int, const ffpa::FwdArgs&, hipStream_t);
typedef void (*config_fn)(int, int*, int*, int*);

struct DimEntry {
  int d;
  launch_fn launch;
  config_fn config;
};

const DimEntry kDims[] = {
#define FFPA_ROW(D) {D, &ffpa::launch_fwd_d##D, &ffpa::tile_config_d##D},
    FFPA_FOR_EACH_HEAD_DIM(FFPA_ROW)
#undef FFPA_ROW
};

// the packed-sequence kernel and its paged-KV twin: one launcher each per head dim of the 16x16x32 build (ffpa_varlen_inst.hip, ffpa_paged_inst.hip)
typedef int (*varlen_fn)(int, int, const ffpa::FwdArgs&, const ffpa::VarlenArgs&, hipStream_t);
typedef int (*paged_fn)(int, int, const ffpa::FwdArgs&, const ffpa::VarlenArgs&, const ffpa::PagedArgs&, hipStream_t);
struct VarlenEntry {
  int d;
  varlen_fn launch;
  paged_fn paged;
};
const VarlenEntry kVarlenDims[] = {
#define FFPA_ROW(D) {D, &ffpa::launch_varlen_d##D, &ffpa::launch_paged_d##D},
    FFPA_FOR_EACH_VARLEN_HEAD_DIM(FFPA_ROW)
#undef FFPA_ROW
};

// Head dims are instantiated in multiples of 64; any multiple of 8 up to 1024 runs on the next instantiation with the
// columns past the caller's head dim read as zeros and never stored (the reference pads to its compiled multiples on
// the host, csrc/cuffpa/ffpa_api.cc:123-161).
int kernel_head_dim(int d) { return (d + 63) / 64 * 64; }

const DimEntry* find_dim(int d) {
  if (d <= 0 || d % 8 != 0) return nullptr;
  const int dk = kernel_head_dim(d);
  for (const DimEntry& e : kDims)
    if (e.d == dk) return &e;
  return nullptr;
}

// Launch plan: which tile variant, and over how many workgroups the KV axis is split.
struct Plan {
  int variant, br, bc, lds, nqt, nt, splits, tiles_per_split;
  int btile;  // 1: a bias with a row axis goes through LDS tiles staged one KV step ahead
  int m16;    // 1: the launch runs ffpa_fwd_m16_kernel (prefill tiles, head dim >= FFPA_M16_MIN_D), 0: ffpa_fwd_split_d_kernel
  int wide;   // 1: ... its wide-row tile, ffpa_fwd_m16w_kernel (launch variant 3)
  int mk;     // m16: the mask kind of the build (0 none, 1 additive bias, 2 boolean mask / ranges)
  int bias_raw;  // FwdArgs.bias_cache_raw
  int bias_lds;  // FwdArgs.bias_lds: > 0 bytes of the key-bias row cache, < 0 -(bytes of the bias-tile staging areas), 0 neither
  int pair;      // 1: row tiles i and nqt - 1 - i share a workgroup (FwdArgs.pair_tiles): the grid holds (nqt + 1) / 2 workgroups per (batch, head)
  int chunk;     // > 1: a causal GQA launch in the HEAD-CHUNK order — (head chunk, batch, row tile, head in chunk), chunks of this many heads of one KV group: the same row
                 //      tile of the group's heads runs at the same time on the same keys (ffpa_fwd_m16_varlen_kernel in its dense mode: the packed-sequence kernel's order)
  int tile_ranges;  // 1: a causal launch whose KV splits are PER ROW TILE — every row tile shares out the KV tiles up to its own diagonal (the same kernel's dense mode)
  size_t ws_bytes;
};

// Per-device facts, looked up once per device and process (write-once caches: the only state the library keeps;
// std::atomic so that concurrent first calls from several host threads are race-free).
constexpr int kMaxDevices = 64;
std::atomic<int> g_cu_count[kMaxDevices];  // 0 = not looked up yet
std::atomic<int> g_arch_ok[kMaxDevices];   // 0 = not looked up yet, 1 = gfx950, 2 = something else

// FFPA_HIP_FAKE_CUS=<n> makes the launch plan price a device of n compute units — a SUPPORTED override: a process that owns a CU-masked
// slice of the GPU (HSA_CU_MASK, partition modes) still reads the whole chip's count from the attribute below; the plan fuzz of tests/test_fwd_gpu.py and
// the CPU plan tables of tests/test_capi.py walk 128 / 256 / 304 with it.  Read on every call while set (no cached state to go stale); the kernels never
// see it — any grid is correct on any device, the plan only decides how fast.
int device_cu_count() {
  if (const char* fake = getenv("FFPA_HIP_FAKE_CUS")) {
    const int n = atoi(fake);
    if (n > 0) return n;
  }
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 256;
  int n = g_cu_count[dev].load(std::memory_order_relaxed);
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    g_cu_count[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

// What the split pricing needs to know about the device besides its CU count: the matrix rate of ONE compute unit and the HBM bandwidth — both read
// from the device (engine clock; memory clock x bus width) instead of being MI355X constants, scaled by what this library's kernels were MEASURED to
// sustain of them on gfx950 (PlanTunables below: the same fractions the bench lines report as roofline.frac).  A part with other
// clocks or another stack count prices itself; without a device (plan queries on a CPU box) the MI355X figures are the fallback.
struct DeviceRates {
  double cu_flops;   // dense bf16 MFMA peak of one CU: 4 SIMDs x 1024 FLOP / clk x engine clock
  double hbm_bytes;  // HBM peak, bytes / s
};
// (one word per device — engine clock in kHz << 32 | HBM bandwidth in MB / s —, so that a concurrent first caller sees both figures or neither)
std::atomic<unsigned long long> g_rates[kMaxDevices];  // 0 = not looked up yet

DeviceRates device_rates() {
  DeviceRates r = {4.0 * 1024.0 * 2.4e9, 8.0e12};  // MI355X: 2.4 GHz, 8 TB/s (MI355X_MICROARCH.md)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) {
    (void)hipGetLastError();
    return r;
  }
  unsigned long long packed = g_rates[dev].load(std::memory_order_acquire);
  if (packed == 0) {
    int clk = 0, mclk = 0, bus = 0;
    long long mbps = 0;
    if (hipDeviceGetAttribute(&clk, hipDeviceAttributeClockRate, dev) != hipSuccess || clk <= 0) clk = 2400000;
    // HBM3 / HBM3E (every gfx94x / gfx950 part; this library only loads on gfx950): four transfers per reported memory clock x bus width —
    // MI355X: 2000 MHz x 8192 bit x 4 / 8 = 8.19 TB/s, MI300X: 1300 MHz -> 5.3 TB/s.  A driver that does not report them leaves the MI355X figure
    if (hipDeviceGetAttribute(&mclk, hipDeviceAttributeMemoryClockRate, dev) == hipSuccess && mclk > 0 &&
        hipDeviceGetAttribute(&bus, hipDeviceAttributeMemoryBusWidth, dev) == hipSuccess && bus > 0)
      mbps = (long long)(4.0 * (double)mclk * 1e3 * (double)bus / 8.0 / 1e6);
    if (mbps < 500000 || mbps > 20000000) mbps = 8000000;  // (0.5 ... 20 TB/s: anything else is a driver reporting another unit)
    (void)hipGetLastError();
    packed = ((unsigned long long)(unsigned)clk << 32) | (unsigned long long)(unsigned)mbps;
    g_rates[dev].store(packed, std::memory_order_release);
  }
  r.cu_flops = 4.0 * 1024.0 * (double)(packed >> 32) * 1e3;
  r.hbm_bytes = (double)(packed & 0xffffffffull) * 1e6;
  return r;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The launch plan.  Every FITTED number it uses lives in this one block, keyed by architecture (this library holds gfx950 code objects only:
// one entry); the rules that use them are a table further down, each with its predicate, its candidates, its margin and the file under
// profiles/ that justifies it.
// ------------------------------------------------------------------------------------------------------------------------------------
struct PlanTunables {
  // fraction of a CU's MFMA peak one workgroup of the prefill tiles sustains while it walks KV tiles (D <= 512 / split-D tiles), and the fraction of
  // the HBM peak the partial-write + merge traffic of a KV-split launch moves at (5.0 / 4.0 TFLOP/s per CU, 5 TB/s on MI355X: profiles/r04_launch_side.txt)
  double tile_rate_frac_d512, tile_rate_frac_splitd, merge_bw_frac;
  double fixed_tiles;          // per-workgroup fixed cost (prologue, epilogue, dispatch) in KV-tile times (profiles/r04_launch_side.txt)
  double max_auto_ws_bytes;    // the pricing never asks a caller for more scratch than this on its own (a forced num_splits may)
  double wide_gain;            // rows per unit time, wide-row tile : 32-row tile — the low end of the measured 2 ... 7 % (profiles/r05_wide_tile.txt)
  int wide_min_wg_per_cu;      // ragged launches (causal flag, masks, ranges): workgroups per CU from which the wide tile is taken (profiles/r05_wide_tile.txt)
  int min_tiles_prefill, min_tiles_short;  // KV tiles a split range holds at least: the merge stays cheap (profiles/r03_decode_splits.txt, r04_launch_side.txt)
  int short_one_per_cu_min_d, short_one_per_cu_lds;  // short-query tiles that want ONE workgroup per CU: head dims from here up, or tiles above this much LDS (profiles/r03_decode_splits.txt)
  int det_tiles_per_split;     // FFPA_FLAG_DETERMINISTIC: KV tiles per split range of a short-query launch (a function of the KV length alone)
  int pair_max_row_tiles;      // causal launches pair row tiles i and n - 1 - i in one workgroup up to this many row tiles per head (profiles/r06_pair_tiles.txt)
  // KV splits of the packed-sequence call (varlen_plan; profiles/r06_varlen_splits.txt): a batch of several sequences is ragged, and ranges beyond "one workgroup per
  // slot" even out what the longest sequence would otherwise run alone — up to this many workgroups per slot, at least this many KV tiles of the longest sequence per
  // range, and partials (written + read back) of at most this fraction of the K + V bytes the launch side can estimate
  int varlen_balance_wgs, varlen_balance_min_tiles;
  double varlen_partial_frac;
  // per-row-tile KV ranges of dense causal launches of one round (pick_tile_ranges; profiles/r06_tile_ranges.txt): keys a range of the average row tile keeps at
  // least (head dims <= 512 / the split-D tiles), and the head dim below which the launch takes three ranges instead of two (two workgroups fit a CU there)
  double tile_ranges_min_keys, tile_ranges_min_keys_splitd;
  int tile_ranges_three_below_d;
};
constexpr PlanTunables kPlanGfx950 = {
    5.0e12 / 9.8304e12, 4.0e12 / 9.8304e12, 5.0e12 / 8.0e12,
    4.0,
    1024.0 * 1048576.0,
    1.04,
    8,
    8, 4,
    320, 80 * 1024,
    16,
    32,
    4, 16,
    0.02,
    640.0, 2048.0,
    256,
};
constexpr const PlanTunables& kT = kPlanGfx950;

// FFPA_OK iff the current device is a gfx950 (the only target of the embedded code objects)
int check_device() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();
    return fail(FFPA_ERR_NO_DEVICE, "no current HIP device");
  }
  int ok = (dev >= 0 && dev < kMaxDevices) ? g_arch_ok[dev].load(std::memory_order_relaxed) : 0;
  if (ok == 0) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) {
      (void)hipGetLastError();
      return fail(FFPA_ERR_NO_DEVICE, "hipGetDeviceProperties(%d) failed", dev);
    }
    ok = strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : 2;
    if (dev >= 0 && dev < kMaxDevices) g_arch_ok[dev].store(ok, std::memory_order_relaxed);
    if (ok == 2) return fail(FFPA_ERR_NO_DEVICE, "device %d is %s: this library holds gfx950 (MI355X) kernels only", dev, prop.gcnArchName);
  }
  if (ok == 2) return fail(FFPA_ERR_NO_DEVICE, "device %d is not a gfx950 (MI355X)", dev);
  return FFPA_OK;
}

// What every rule of the plan looks at: the call, the tile the launch would run, the device, and the pricing model's inputs.
struct PlanCtx {
  const ffpa_fwd_params* p;
  const DimEntry* de;
  Plan* pl;
  int64_t cus, base;     // compute units; workgroups of the unsplit launch (batch x heads x row tiles)
  int dk;                // head dim of the kernel instantiation
  double nt_eff;         // KV tiles an average row tile walks (causal flag: up to its diagonal)
  int nt_visible;        // KV tiles any row can see: a split range past them would be workgroups that do nothing
  double tile_s, out_elems, merge_bw;
  bool priced;           // the split count is the pricing's to choose (prefill tile, no forced count, scratch offered)
  bool deterministic;    // FFPA_FLAG_DETERMINISTIC
};

// The pricing model of a prefill launch split over s KV ranges (round 4, profiles/r04_launch_side.txt; it over-prices the splits by ~ 10 % on every measured shape):
//   time(s) = rounds(s) x (tiles per split + fixed_tiles of per-workgroup fixed cost) x tile time  +  (8 s + 2) bytes per output element / merge bandwidth
double predicted(const PlanCtx& c, int64_t s) {
  const double rounds = (double)((c.base * s + c.cus - 1) / c.cus);
  return rounds * (c.nt_eff / s + kT.fixed_tiles) * c.tile_s + (s > 1 ? c.out_elems * (8.0 * s + 2.0) / c.merge_bw : 0.0);
}
// a split count is admissible for the pricing's own rules if its last KV range still holds keys some row can see and its scratch stays under the cap
bool admissible(const PlanCtx& c, int64_t s) {
  const int64_t tps = (c.pl->nt + s - 1) / s;
  return (s - 1) * tps < c.nt_visible && (double)s * c.out_elems / c.dk * (c.dk + 1.0) * 4.0 <= kT.max_auto_ws_bytes;
}

// A PRICED rule: where `applies`, every split count of `range` (ascending; the walk stops at the first count that leaves a range fewer than
// min_tiles_prefill KV tiles) is priced against the count the plan holds so far, and the cheapest one that beats `margin` x that price is taken.
struct PricedRule {
  const char* name;
  bool (*applies)(const PlanCtx&, int64_t cur);
  void (*range)(const PlanCtx&, int64_t cur, int64_t* lo, int64_t* hi);
  double margin;
  const char* evidence;
};
int64_t run_priced(const PlanCtx& c, const PricedRule& r, int64_t cur) {
  if (!r.applies(c, cur)) return cur;
  int64_t lo = 0, hi = -1, pick = cur;
  r.range(c, cur, &lo, &hi);
  const double t0 = predicted(c, cur);
  double best = t0;
  for (int64_t s = lo; s <= hi; ++s) {
    if (c.pl->nt / s < kT.min_tiles_prefill) break;
    if (!admissible(c, s)) continue;
    const double t = predicted(c, s);
    if (t < r.margin * t0 && t < best) best = t, pick = s;
  }
  return pick;
}
const PricedRule kRaggedRound = {
    // a prefill launch of a little over one round of workgroups — 288 ... 384 on 256 CUs — takes two rounds' time.  Split over 2 or 3 KV ranges it fills whole
    // rounds (9 heads x 32 row tiles x 3 = 864 = 3.4 rounds), and on a long context the partials and their merge cost little next to that: B1 H9 / H10 / H11 /
    // H12 x Nq 4096 x Nkv 8192 D512 + 18 / + 15 / + 10 / + 5 %, H40 x Nq 1024 + 14 %, D = 1024 H5 + 19 %; against 2048 keys or under the causal flag the same
    // splits LOSE 18 ... 37 % — the rule prices both sides and splits only for a predicted gain of 10 %.  The same pricing serves a launch of PART of a round
    // (CUs / 2 < workgroups < CUs): 160 workgroups in three KV ranges are 480 = two rounds of a third of the length — B1 H5 x Nq 4096 D512 + 10 % at 8192 keys,
    // + 19 % at 16384, D = 320 + 7 %, H20 x Nq 1024 + 8 %; 192 and 224 workgroups (H6, H7, D = 1024 H3) gain from no split count, and the model picks none.
    "ragged round",
    [](const PlanCtx& c, int64_t) {
      return c.priced && 2 * c.base > c.cus && 2 * c.base <= 3 * c.cus && c.p->bias == nullptr && c.p->kv_bounds == nullptr && !(c.p->dropout_p > 0.f);
    },
    [](const PlanCtx&, int64_t, int64_t* lo, int64_t* hi) { *lo = 2, *hi = 3; },
    0.9, "profiles/r04_launch_side.txt"};
const PricedRule kTwoRounds = {
    // under-filled launches whose CUs / workgroups is far from a whole number (96 workgroups: two ranges fill 192 of 256 CUs): a count that makes two rounds of
    // shorter workgroups can beat the one-round count on a long context — 96 workgroups x 5 = 480: + 6 ... 11 % at 16384 keys, + 7 % at D = 1024 / 8192 keys,
    // + 2 % at D = 512 / 8192 keys; 80 x 3 and 56 x 4 stay.  Both sides pay partials and a merge, so the margin is 5 % here.
    "two rounds of shorter workgroups",
    [](const PlanCtx& c, int64_t cur) { return c.priced && c.base * 2 <= c.cus && cur >= 2; },
    [](const PlanCtx&, int64_t cur, int64_t* lo, int64_t* hi) { *lo = cur + 1, *hi = 3 * cur < ffpa::kMergeMaxSplits ? 3 * cur : ffpa::kMergeMaxSplits; },
    0.95, "profiles/r04_launch_side.txt"};

// The wide-row prefill tile (ffpa_fwd_m16w_kernel.h: 16 RH rows per wave, RH sized to the accumulator file; 64-key tiles, double-buffered, one barrier
// per KV step): does this launch take it?  The builds that exist: no additive bias, no dropout.  Measured on D = 320 (profiles/r05_wide_tile.txt, interleaved
// same-box A/B): a row of the 192-row tile costs 2 ... 7 % less than a row of the 128-row tile, so what decides is how the launch quantises into rounds of
// workgroups — B2 Hq32 x Nq 8192 (config 4 without its mask): 2752 workgroups = 11 rounds of 192 rows against 16 of 128: + 2.3 %; B1 H32 x Nq 8192: 1376 =
// 5.4 -> SIX rounds against 8: - 4 %.  Launches whose workgroups differ in length (causal flag, masks, mask ranges: longest first, the last round's tail is short
// workgroups) have no such quantum but need enough workgroups per CU for the lengths to even out: config 4 (10.75 per CU) + 1.0 ... 1.6 %, B1 H32 causal 8192
// (5.4 per CU) - 3 %.
bool pick_wide_tile(const ffpa_fwd_params* p, const DimEntry* de, const Plan& pl, int64_t cus) {
  if (pl.variant != 0 || (p->flags & (FFPA_FLAG_DEBUG_SAFE_PATH | FFPA_FLAG_NO_WIDE_TILE | FFPA_FLAG_DETERMINISTIC))) return false;
  if (p->dropout_p > 0.f || !(p->bias == nullptr || p->bias_dtype == FFPA_BIAS_BOOL8)) return false;
  int br = 0, bc = 0, lds = 0;
  de->config(3, &br, &bc, &lds);
  if (br <= 0) return false;
  if (p->flags & FFPA_FLAG_WIDE_TILE) return true;
  const int64_t wgs_wide = (int64_t)p->batch * p->heads_q * ((p->seqlen_q + br - 1) / br);
  const int64_t wgs_now = (int64_t)p->batch * p->heads_q * ((p->seqlen_q + pl.br - 1) / pl.br);
  if (p->causal || p->bias != nullptr || p->kv_bounds != nullptr) return wgs_wide >= kT.wide_min_wg_per_cu * cus;
  if (wgs_wide < 2 * cus) return false;  // (launches of a round or two: the KV-split rules were measured on the 128-row tile)
  const double t_wide = (double)((wgs_wide + cus - 1) / cus) * br / kT.wide_gain, t_now = (double)((wgs_now + cus - 1) / cus) * pl.br;
  return t_wide < t_now;
}

// The pricing's inputs for this call (`pl` holds variant, tile and tile counts already).
PlanCtx plan_context(const ffpa_fwd_params* p, const DimEntry* de, Plan* pl, int64_t cus) {
  PlanCtx c = {};
  c.p = p, c.de = de, c.pl = pl, c.cus = cus;
  c.base = (int64_t)p->batch * p->heads_q * pl->nqt;
  c.dk = kernel_head_dim(p->head_dim);
  // KV tiles an average row tile walks: all of them — or, under the causal flag, those up to its diagonal: rows r see keys <= r + causal_offset, the mean
  // over the rows is causal_offset + Nq / 2, clamped to [0, Nkv] (top-left causal against a long context: Nq / 2 keys, not Nkv / 2; tail-aligned: Nkv - Nq / 2)
  c.nt_eff = (double)pl->nt;
  int64_t visible_end = p->seqlen_kv;  // keys at and past this index are hidden from EVERY row of the launch
  if (p->causal) {
    double mean = (double)p->causal_offset + 0.5 * (double)(p->causal_row_mod ? p->causal_row_mod : p->seqlen_q);
    mean = mean < 0.0 ? 0.0 : (mean > (double)p->seqlen_kv ? (double)p->seqlen_kv : mean);
    c.nt_eff = mean / pl->bc > 1.0 ? mean / pl->bc : 1.0;
    const int64_t last = (int64_t)(p->causal_row_mod ? p->causal_row_mod : p->seqlen_q) - 1 + p->causal_offset + 1;
    visible_end = last < 0 ? 0 : (last < p->seqlen_kv ? last : p->seqlen_kv);
  }
  c.nt_visible = (int)((visible_end + pl->bc - 1) / pl->bc);
  const DeviceRates rates = device_rates();
  c.tile_s = 4.0 * pl->br * pl->bc * c.dk / ((c.dk > 512 ? kT.tile_rate_frac_splitd : kT.tile_rate_frac_d512) * rates.cu_flops);  // one KV tile of one workgroup
  c.out_elems = (double)p->batch * p->heads_q * p->seqlen_q * c.dk;
  c.merge_bw = kT.merge_bw_frac * rates.hbm_bytes;
  c.deterministic = (p->flags & FFPA_FLAG_DETERMINISTIC) != 0;
  c.priced = pl->variant == 0 && !(p->flags & (FFPA_FLAG_DEBUG_SAFE_PATH | FFPA_FLAG_FORCE_SPLITS | FFPA_FLAG_DETERMINISTIC)) && p->num_splits == 0 && p->workspace != nullptr;
  return c;
}

// KV-split launches (partials + LSE merge): over how many KV ranges?  Short-query tiles: occupancy heuristic cf. select_decode_num_splits
// (native/launch.cuh:17-67) — aim at one (head dims >= 320) or two workgroups per CU, at least 4 KV tiles per split so the merge stays cheap.  Prefill tiles
// split when the launch would leave more than half of the chip idle (chunked prefill against a long context with few heads per GPU: one workgroup per CU, at
// least 8 KV tiles per split), or when a priced rule says so.
int64_t pick_splits(const PlanCtx& c) {  // (0: this launch does not split — no clamp applies)
  const ffpa_fwd_params* p = c.p;
  const Plan& pl = *c.pl;
  if (c.deterministic) {
    // batch-invariant bits: a prefill launch never splits; a short-query launch splits by the KV length ALONE (a fixed number of tiles per range) — the
    // plan of a (batch, head) slice then does not depend on how many slices share the launch, and neither does a single bit of its output
    if (pl.variant == 0 || p->num_splits == 1) return 0;
    return (pl.nt + kT.det_tiles_per_split - 1) / kT.det_tiles_per_split;
  }
  const bool forced = pl.variant == 0 && (p->flags & FFPA_FLAG_FORCE_SPLITS) && p->num_splits > 1;  // (the flag: sweeps of the rules, tools/gpu_prefill_splits.py)
  const int64_t ragged = run_priced(c, kRaggedRound, 1);
  const bool underfilled = pl.variant == 0 && !(p->flags & FFPA_FLAG_DEBUG_SAFE_PATH) && (c.base * 2 <= c.cus || ragged > 1 || forced);
  if (!((pl.variant == 1 || underfilled) && p->num_splits != 1)) return 0;
  // short-query tiles, measured (tools/gpu_decode_splits.py, profiles/r03_decode_splits.txt): head dims >= 320 want ONE workgroup per CU — their tiles are
  // 20 KiB and up, one workgroup keeps enough bytes in flight, and half the splits are half the partials to write and merge (- 3 ... 14 % per step
  // against two per CU; rounded DOWN: at most two of these workgroups fit a CU, above D = 512 one, and a launch a little over one per CU takes twice
  // as long as one a little under) — the small head dims two (8 KiB tiles at D = 128: one per CU is 40 ... 60 % slower, three or four 10 ... 25 %)
  const bool sq_one_per_cu = c.dk >= kT.short_one_per_cu_min_d || pl.lds > kT.short_one_per_cu_lds;  // (or tiles of which only one workgroup fits a CU)
  int64_t want = pl.variant == 1 ? (sq_one_per_cu ? c.cus / c.base : (2 * c.cus + c.base - 1) / c.base) : c.cus / c.base;
  if (forced) want = p->num_splits;
  if (ragged > 1) want = ragged;
  want = run_priced(c, kTwoRounds, want);
  return want < 1 ? 1 : want;
}

// What every split count is clamped by, whoever chose it: tiles per range, ranges nobody can see, the merge kernel's LDS, the caller's request and scratch.
int64_t clamp_splits(const PlanCtx& c, int64_t want) {
  const ffpa_fwd_params* p = c.p;
  const Plan& pl = *c.pl;
  const int min_tiles = pl.variant == 1 ? kT.min_tiles_short : kT.min_tiles_prefill;
  const int64_t cap = pl.nt / min_tiles > 0 ? pl.nt / min_tiles : 1;
  if (want > cap) want = cap;
  // prefill under the causal flag: no KV range entirely behind every row's diagonal (top-left causal against a long context: rows see at most Nq keys —
  // ranges past them would be workgroups that do nothing, their partials and the merge pure cost)
  if (pl.variant == 0 && !(p->flags & FFPA_FLAG_FORCE_SPLITS))
    while (want > 1 && (want - 1) * ((pl.nt + want - 1) / want) >= c.nt_visible) --want;
  if (want > ffpa::kMergeMaxSplits) want = ffpa::kMergeMaxSplits;  // the merge kernel keeps the split weights in LDS
  if (p->num_splits > 1 && want > p->num_splits) want = p->num_splits;
  if (want < 1) want = 1;
  const size_t per_split = (size_t)p->batch * p->heads_q * p->seqlen_q * ((size_t)c.dk + 1) * sizeof(float);
  if (p->workspace == nullptr) want = 1;
  else if ((uint64_t)want * per_split > p->workspace_bytes) want = (int64_t)(p->workspace_bytes / per_split);
  return want < 1 ? 1 : want;
}

// The 16x16x32 prefill build of this call (ffpa_fwd_inst.hip): no bias / boolean masks and mask ranges / additive biases (and anything next to dropout) — and,
// for an additive bias, where the initial S^T accumulators come from (an LDS row cache, a ring, staged tiles, or element loads).
void pick_m16_build(const ffpa_fwd_params* p, const DimEntry* de, Plan& pl, int dk) {
  const bool no_bias = p->bias == nullptr && p->kv_bounds == nullptr;
  const bool additive = p->bias != nullptr && p->bias_dtype >= FFPA_BIAS_FP16 && p->bias_dtype <= FFPA_BIAS_FP32;
  pl.mk = no_bias ? 0 : ((additive || p->dropout_p > 0.f) ? 1 : 2);
  if (pl.mk != 1) return;
  // 64-key tiles at every head dim <= 512 (the LDS also holds the bias)
  de->config(2, &pl.br, &pl.bc, &pl.lds);
  pl.nt = (p->seqlen_kv + pl.bc - 1) / pl.bc;
  const int esz = p->bias_dtype == FFPA_BIAS_FP32 ? 4 : 2;
  const int stagers = dk > 512 ? 2 : 4;  // waves that carry a bias tile (D > 512: one of the two waves of a row block)
  const bool lds_ok = additive && pl.splits == 1 && !(p->flags & FFPA_FLAG_NO_BIAS_LDS);
  const int64_t cache = (int64_t)pl.nt * pl.bc * 4;  // a key bias as fp32 / scale, a whole number of tiles
  const int64_t stage = (int64_t)stagers * 32 * pl.bc * esz;
  bool stage_ok = lds_ok && p->bias_stride[3] == 1 && reinterpret_cast<uintptr_t>(p->bias) % 16 == 0 && p->bias_stride[2] < (1LL << 24) &&
                  pl.lds + stage <= 160 * 1024;
  for (int i = 0; i < 3 && stage_ok; ++i) stage_ok = (p->bias_stride[i] * esz) % 16 == 0;
  const bool cache16 = esz == 2 && pl.lds + cache / 2 <= 160 * 1024;  // ... or as the caller's 16-bit elements, converted per step
  // split-D tiles with the softmax pipeline (D > 512, D % 128 == 0), nothing but a key bias: the key-bias build runs the pipeline too (round 5); its LDS is the
  // unmasked build's (6 KiB of exchange per wave) + a RING of fp32 bias entries — a power of two, at least 2048 (all D = 1024 has left), refilled half a ring
  // at a time 1024+ keys ahead of the walk (ffpa_fwd_m16_kernel.h)
  const bool ring = lds_ok && p->bias_stride[2] == 0 && dk > 512 && dk % 128 == 0 && p->kv_bounds == nullptr && !(p->dropout_p > 0.f);
  if (ring) {
    int br0 = 0, bc0 = 0, lds0 = 0;
    de->config(4, &br0, &bc0, &lds0);
    int bytes = 8192;
    while (2 * bytes <= 160 * 1024 - lds0 && bytes < 65536) bytes *= 2;
    pl.lds = lds0;
    pl.bias_raw = 0;
    pl.bias_lds = bytes;
    pl.mk = 3;
  } else if (lds_ok && p->bias_stride[2] == 0 && (pl.lds + cache <= 160 * 1024 || cache16)) {
    pl.bias_raw = pl.lds + cache <= 160 * 1024 ? 0 : 1;
    pl.bias_lds = (int)(pl.bias_raw ? cache / 2 : cache);
    if (p->kv_bounds == nullptr && !(p->dropout_p > 0.f)) pl.mk = 3;  // nothing but a cached key bias: the lean key-bias build
  } else if (stage_ok) {
    pl.btile = 1;
    pl.bias_lds = -(int)stage;
  }
}

// 32x32x16 build (head dims <= 64): a 16-bit bias with a real row axis is staged through LDS by LDS-DMA one KV step ahead
// (4 waves x [32 rows x 64 keys]); those launches run the build with 64-key tiles at every head dim (tile config variant 2)
void pick_small_d_bias_tiles(const ffpa_fwd_params* p, const DimEntry* de, Plan& pl) {
  if (pl.m16 || pl.variant != 0 || pl.splits != 1 || p->bias == nullptr || p->bias_stride[2] == 0 || p->bias_stride[3] != 1) return;
  if (!(p->bias_dtype == FFPA_BIAS_FP16 || p->bias_dtype == FFPA_BIAS_BF16) || (p->flags & (FFPA_FLAG_NO_BIAS_LDS | FFPA_FLAG_DEBUG_SAFE_PATH)) || p->dropout_p > 0.f) return;
  bool ok = reinterpret_cast<uintptr_t>(p->bias) % 16 == 0 && p->bias_stride[2] < (1LL << 24);
  for (int i = 0; i < 3; ++i) ok = ok && (p->bias_stride[i] * 2) % 16 == 0;
  int br = 0, bc = 0, lds = 0;
  de->config(2, &br, &bc, &lds);
  if (!(ok && lds + 4 * 32 * bc * 2 <= 160 * 1024)) return;
  pl.btile = 1;
  pl.br = br, pl.bc = bc, pl.lds = lds;
  pl.nt = (p->seqlen_kv + pl.bc - 1) / pl.bc;
}

// Paired row tiles (ffpa_fwd_m16_kernel.h, FwdArgs::pair_tiles): under the causal flag workgroup i of a head walks row tile nqt - 1 - i and then row tile i — equal
// work per workgroup, half the dispatches, bit-identical outputs.  The builds that can: the 16x16x32 prefill kernel (not its wide-row tile), unsplit, no bias /
// ranges / packed rows.  Measured (interleaved same-box A/B over 19 causal shapes, profiles/r06_pair_tiles.txt): what it buys is the launch's TAIL — the last
// round of an unpaired launch is its short workgroups, most of a CU's time there is idle — so it pays where a head has FEW row tiles: 16 tiles (B4 H32 N 2048 D512)
// + 2 ... 12.7 % (three boxes), 32 tiles 0 ... + 3.6 % (D512) / + 2 ... 7.1 % (D320), 64 tiles - 1 ... + 2.4 % (D 128 ... 768; D = 1024 N 4096 + 0.3 %: not taken), 96 tiles - 0.9 %,
// 128 tiles - 1.2 % (D512 N 16384) ... - 7 / - 9 % (D = 1024 N 8192) — and only where the diagonal makes tiles unequal (tail-aligned causal against a context four
// times the query: - 3.1 %).  The rule: up to 32 row tiles per head.
bool pick_pair_tiles(const ffpa_fwd_params* p, const Plan& pl) {
  if (!pl.m16 || pl.wide || pl.splits != 1 || !p->causal || p->bias != nullptr || p->kv_bounds != nullptr || p->causal_row_mod != 0 || pl.nqt < 2) return false;
  if (p->flags & (FFPA_FLAG_NO_PAIR_TILES | FFPA_FLAG_DEBUG_SAFE_PATH)) return false;
  if (p->flags & FFPA_FLAG_PAIR_TILES) return true;
  // keys the first / the last row tile can see: the pairing evens out what the diagonal makes unequal — at least a factor of two between them
  auto clampkv = [&](int64_t x) { return x < 0 ? (int64_t)0 : (x > p->seqlen_kv ? (int64_t)p->seqlen_kv : x); };
  const int64_t lo = clampkv((int64_t)p->causal_offset + pl.br), hi = clampkv((int64_t)p->causal_offset + p->seqlen_q);
  return pl.nqt <= kT.pair_max_row_tiles && 2 * lo <= hi;
}

// Heads that walk a sequence side by side in the head-chunk order: the largest divisor of the KV group's size that leaves a multiple of eight chunks (every XCD
// then owns whole chunks of every batch element / sequence: balance); 1 = plain head-major order.
int pick_head_chunk(int heads_q, int group) {
  for (int c = group; c > 1; --c)
    if (group % c == 0 && heads_q % c == 0 && (heads_q / c) % 8 == 0) return c;
  return 1;
}

// Causal GQA launches in the head-chunk order (round 6: found on the packed-sequence kernel, whose order it is).  A head's row tiles alone fill an XCD for a round,
// so in the dense order the heads of a KV group stream the group's K / V one after the other; interleaved per row tile they stream it together.  Same tile, same
// bits; interleaved same-run A/B of the two orders on dense shapes (tools/gpu_dense_vs_packed.py, profiles/r06_head_chunks.txt): Hq 32 / Hkv 8 N 8192 causal D 512
// + 3.2 %, D 1024 + 4.3 %, D 320 + 2.8 %, B 2 N 4096 + 1.2 %, B 4 N 2048 + 1.8 % (over the paired-tile launch); non-causal +- 0; MHA - 3.7 % with chunks of 4 heads
// (four K / V streams at once instead of one) -> chunks never span KV groups.  Builds without bias / mask ranges / dropout; every row must see a key (the kernel's
// empty-row contract is the packed call's: 0, not SDPA's NaN).
int pick_dense_head_chunk(const ffpa_fwd_params* p, const Plan& pl, int dk) {
  if (!pl.m16 || pl.wide || pl.splits != 1 || pl.mk != 0 || !p->causal || p->causal_offset < 0 || p->causal_row_mod != 0 || p->dropout_p > 0.f || dk < FFPA_M16_MIN_D) return 1;
  if (p->flags & (FFPA_FLAG_NO_HEAD_CHUNKS | FFPA_FLAG_DEBUG_SAFE_PATH | FFPA_FLAG_PAIR_TILES)) return 1;
  if (p->lse != nullptr && (int64_t)p->batch * p->heads_q * p->seqlen_q >= (1LL << 31)) return 1;
  return pick_head_chunk(p->heads_q, p->heads_q / p->heads_kv);
}

// PER-ROW-TILE KV ranges for causal launches of ONE ROUND of workgroups (CUs / 2 < workgroups <= CUs: a whole prompt with a few heads per GPU — 8 heads x 4096
// tokens are 256 row tiles).  Longest first, the round ends on a few long row tiles while the short ones' CUs idle; uniform KV ranges (the dense kernel's) do not help —
// a short row tile sees nothing of the later ranges, the long ones still walk the first range whole: 2 ranges - 15 %, tools/gpu_prefill_splits.py c_* —, ranges of
// every row tile's OWN visible keys do (the packed-sequence kernel computes them on the device: its dense mode): 8 heads x 4096 x 4096 D 512 187 -> 165 us against
// 199 us of the paired-tile launch, D 128 85 -> 70 us (profiles/r06_tile_ranges.txt).  Taken when the longest row tile walks >= 1.5 x the average one and a range
// of the average one keeps enough keys (below).  The builds the dense mode has (pick_dense_head_chunk); fp32 partials + merge: equal to the one-range launch
// to rounding — FFPA_FLAG_DETERMINISTIC / num_splits = 1 / FFPA_FLAG_NO_TILE_RANGES keep one range.
int pick_tile_ranges(const ffpa_fwd_params* p, const Plan& pl, const PlanCtx& c) {
  if (!pl.m16 || pl.wide || pl.splits != 1 || pl.mk != 0 || !p->causal || p->causal_offset < 0 || p->causal_row_mod != 0 || p->dropout_p > 0.f || c.dk < FFPA_M16_MIN_D) return 0;
  if (p->flags & (FFPA_FLAG_NO_TILE_RANGES | FFPA_FLAG_DEBUG_SAFE_PATH | FFPA_FLAG_PAIR_TILES | FFPA_FLAG_DETERMINISTIC)) return 0;
  if (p->workspace == nullptr || p->num_splits == 1 || pl.nqt < 2) return 0;
  if ((int64_t)p->batch * p->heads_q * p->seqlen_q >= (1LL << 31)) return 0;
  int64_t want = 0;
  if ((p->flags & FFPA_FLAG_TILE_RANGES) && (p->flags & FFPA_FLAG_FORCE_SPLITS) && p->num_splits > 1) {
    want = p->num_splits < pl.nt ? p->num_splits : pl.nt;  // (sweeps and tests: exactly n)
  } else if (c.priced && 2 * c.base > c.cus && c.base <= c.cus && (double)c.nt_visible >= 1.5 * c.nt_eff) {
    // a range of the average row tile keeps at least tile_ranges_min_keys keys (the partials and their merge: measured neutral at 512 keys per range — 16 heads x
    // 2048 x 2048 - 1 % —, + 22 % at 750, + 15 ... 33 % at 1024; the split-D tiles - 4 % at 1024, + 8 % at 2048); small tiles (two workgroups per CU) take three
    const double avg_keys = c.nt_eff * pl.bc, min_keys = c.dk > 512 ? kT.tile_ranges_min_keys_splitd : kT.tile_ranges_min_keys;
    for (int64_t w = c.dk < kT.tile_ranges_three_below_d ? 3 : 2; w >= 2 && want == 0; --w)
      if (avg_keys / (double)w >= min_keys) want = w;
  }
  if (want > ffpa::kMergeMaxSplits) want = ffpa::kMergeMaxSplits;
  const size_t per_split = (size_t)p->batch * p->heads_q * p->seqlen_q * ((size_t)c.dk + 1) * sizeof(float);
  if ((uint64_t)want * per_split > p->workspace_bytes) want = (int64_t)(p->workspace_bytes / per_split);
  return want > 1 ? (int)want : 0;
}

// Launch plan: tile variant -> wide-row tile? -> KV splits (rules above) -> build and bias placement -> scratch.
Plan make_plan(const ffpa_fwd_params* p, const DimEntry* de) {
  Plan pl = {};
  // <= 32 query rows per (batch, head): one 32-row block per workgroup with D split over all four waves;
  // the reference switches to its split-KV decode kernels only for Nq == 1 (native/launch.cuh:306-340)
  pl.variant = (p->seqlen_q <= 32 && !(p->flags & FFPA_FLAG_DEBUG_SAFE_PATH)) ? 1 : 0;
  de->config(pl.variant, &pl.br, &pl.bc, &pl.lds);
  const int64_t cus = device_cu_count();
  pl.wide = pick_wide_tile(p, de, pl, cus) ? 1 : 0;
  if (pl.wide) de->config(3, &pl.br, &pl.bc, &pl.lds);
  pl.nqt = (p->seqlen_q + pl.br - 1) / pl.br;
  pl.nt = (p->seqlen_kv + pl.bc - 1) / pl.bc;
  const PlanCtx c = plan_context(p, de, &pl, cus);
  const int64_t want = (p->flags & FFPA_FLAG_TILE_RANGES) ? 0 : pick_splits(c);  // (the flag: this launch's ranges are per row tile or none — pick_tile_ranges below)
  pl.splits = want > 0 ? (int)clamp_splits(c, want) : 1;
  pl.m16 = (pl.variant == 0 && !(p->flags & FFPA_FLAG_DEBUG_SAFE_PATH) && c.dk >= FFPA_M16_MIN_D) ? 1 : 0;
  if (pl.m16) pick_m16_build(p, de, pl, c.dk);
  pick_small_d_bias_tiles(p, de, pl);
  pl.chunk = pick_dense_head_chunk(p, pl, c.dk);
  if (const int ranges = pick_tile_ranges(p, pl, c)) {
    pl.tile_ranges = 1;
    pl.splits = ranges;
    if (pl.chunk < 1) pl.chunk = 1;
  }
  pl.pair = (pl.chunk <= 1 && pick_pair_tiles(p, pl)) ? 1 : 0;
  pl.tiles_per_split = (pl.nt + pl.splits - 1) / pl.splits;
  if (pl.tiles_per_split < 1) pl.tiles_per_split = 1;
  if (!pl.tile_ranges) pl.splits = (pl.nt + pl.tiles_per_split - 1) / pl.tiles_per_split;  // (per-row-tile ranges: the kernel sizes them, every count is exact)
  if (pl.splits < 1) pl.splits = 1;
  pl.ws_bytes = pl.splits > 1 ? (size_t)pl.splits * p->batch * p->heads_q * p->seqlen_q * ((size_t)c.dk + 1) * sizeof(float) : 0;
  return pl;
}

// Shape checks shared by the launch and the queries; `launch`: with the launch's own pointer / dtype / head-ratio checks, each at the place in the order the call
// has always reported it.  Returns FFPA_OK or a status.
int check_basic(const ffpa_fwd_params* p, const DimEntry** de_out, bool launch = false) {
  if (p == nullptr) return fail(FFPA_ERR_NULL_POINTER, "params is NULL");
  if (p->struct_size != sizeof(ffpa_fwd_params) || p->abi_version != FFPA_ATTN_ABI_VERSION)
    return fail(FFPA_ERR_BAD_ABI, "ffpa_fwd_params ABI mismatch: size %u (want %zu), version %u (want %d)",
                p->struct_size, sizeof(ffpa_fwd_params), p->abi_version, FFPA_ATTN_ABI_VERSION);
  if (launch && (!p->q || !p->k || !p->v || !p->o)) return fail(FFPA_ERR_NULL_POINTER, "q/k/v/o must be non-NULL");
  if (launch && p->dtype != FFPA_DTYPE_BF16 && p->dtype != FFPA_DTYPE_FP16)
    return fail(FFPA_ERR_BAD_DTYPE, "dtype %d is not bf16(0)/fp16(1)", p->dtype);
  if (p->batch <= 0 || p->heads_q <= 0 || p->heads_kv <= 0 || p->seqlen_q <= 0 || p->seqlen_kv <= 0)
    return fail(FFPA_ERR_BAD_SHAPE, "non-positive dimension: B=%d Hq=%d Hkv=%d Nq=%d Nkv=%d", p->batch, p->heads_q,
                p->heads_kv, p->seqlen_q, p->seqlen_kv);
  if (launch && p->heads_q % p->heads_kv != 0)
    return fail(FFPA_ERR_BAD_SHAPE, "num_heads: Hq=%d is not a multiple of Hkv=%d", p->heads_q, p->heads_kv);
  const DimEntry* de = find_dim(p->head_dim);
  if (de == nullptr)
    return fail(FFPA_ERR_BAD_HEADDIM, "headdim not support! D=%d (supported: multiples of 8 in [8, 1024])", p->head_dim);
  *de_out = de;
  return FFPA_OK;
}

// "Plan as if the caller had unlimited scratch": what the *_workspace_bytes / *_split_tickets queries size for (either parameter struct)
template <typename P>
P with_unlimited_scratch(const P& params) {
  P q = params;
  q.workspace = reinterpret_cast<void*>(16);
  q.workspace_bytes = ~0ull;
  return q;
}

// Dropout keeps the element of Philox word w when u(w) = ((float)w + 1.0f) * 2^-32 > p (prefill.cuh:437-440).  u is monotone in w
// (int -> float conversion and the add both round monotonically), so the decision is w >= T for the smallest kept word T — found here by
// bisection with the very float expression, once per call; the kernels compare integers.  p < 1 (checked) keeps w = 2^32 - 1 (u = 1).
uint32_t dropout_keep_threshold(float p) {
  if (!(p > 0.f)) return 0u;
  auto kept = [p](uint32_t w) { return ((float)w + 1.0f) * 2.3283064365386963e-10f > p; };
  uint32_t lo = 0u, hi = 0xFFFFFFFFu;  // kept(hi) holds; the answer is in [lo, hi]
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (kept(mid)) hi = mid; else lo = mid + 1u;
  }
  return lo;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int check_strides(const char* name, const int64_t* s, int n) {
  for (int i = 0; i < n; ++i) {
    if (s[i] < 0) return fail(FFPA_ERR_BAD_STRIDE, "%s stride[%d]=%lld is negative", name, i, (long long)s[i]);
    if (s[i] % 8 != 0)
      return fail(FFPA_ERR_BAD_STRIDE, "%s stride[%d]=%lld is not a multiple of 8 elements (16 bytes)", name, i,
                  (long long)s[i]);
  }
  return FFPA_OK;
}

// The softmax scale as the 16x16x32 build takes it: it folds the scale into its exponent (needs scale > 0) and takes additive biases in units of 1 / scale: a zero
// scale (scores = bias) reaches it as "Q = 0, scale = 1", a negative one as "-Q, |scale|" — the same scores
void fold_scale(ffpa::FwdArgs& a, float softmax_scale) {
  if (softmax_scale == 0.f) {
    a.scale_log2 = 1.4426950408889634f;
    a.q_mode = 1;
  } else {
    const float mag = fabsf(softmax_scale);  // a negative scale: (-Q, |scale|) — exact, and the kernel's fused exponent needs scale > 0
    a.scale_log2 = mag * 1.4426950408889634f;
    a.inv_scale = (float)(1.0 / (double)mag);
    if (softmax_scale < 0.f) a.q_mode = 2;
  }
}

// XCDs per head (xcd_logical_id, ffpa_common.h).  One XCD per head keeps a head's K/V stream in one L2; but then eight heads are in flight chip-wide,
// and once their K + V no longer fit the Infinity Cache the second and later rounds of a head's row tiles come from HBM instead (config 3: eight heads x
// 32 MiB = the whole 256 MiB).  Launches with at least two rounds of row tiles per head and XCD (`share`: the caller's side of that rule) therefore share a head
// between the smallest power-of-two number of XCDs that brings the K + V in flight under 200 MiB (measured, profiles/r03_xcd_group.txt).  The packed call prices
// the longest sequence the caller announces.
int pick_xcd_group(unsigned flags, bool share, int64_t seqlen_kv, int head_dim) {
  int g = 1;
  const unsigned forced = (flags >> 8) & 7u;
  if (forced != 0) {
    g = 1 << (forced - 1 > 3 ? 3 : forced - 1);
  } else if (share) {
    const double kv_mib = 2.0 * (double)seqlen_kv * (double)head_dim * 2.0 / 1048576.0;  // K + V of one (batch, kv head)
    while (g < 8 && (8 / g) * kv_mib > 200.0) g *= 2;
  }
  return g;
}

// The split-D tiles (D > 512) give a DMA piece less than a microsecond to land (32-key steps, single K / V buffers): their launches touch the
// tile two steps ahead (ffpa_fwd_m16_kernel.h, "L2 prefetch").  Measured, same library with and without (profiles/r03_l2_prefetch.txt):
// D = 576 ... 1024: + 3 ... 9 % (D = 768: +- 0), every shape tried (self, cross, GQA, batch 4, causal, key bias); D <= 512: - 1 ... 2 %, off.
int pick_l2_prefetch(unsigned flags, bool split_d_tiles) {
  return (flags & FFPA_FLAG_NO_L2_PREFETCH) ? 0 : ((flags & FFPA_FLAG_L2_PREFETCH) || split_d_tiles) ? 1 : 0;
}

// What a launcher of ffpa_launch.h returned (0, -1 ... -4, or a hipError_t) as a status + message.  lds >= 0: the message names the LDS size the launch asked
// for; safe_d > 0: -3 is "this build does not exist" for head dim safe_d (the dense call, whose debug twins are built for a few head dims only).
int launch_status(int st, int lds, int safe_d) {
  if (st == 0) return FFPA_OK;
  if (st == -3 && safe_d > 0) return fail(FFPA_ERR_UNSUPPORTED, "debug safe-path kernel is not built for D=%d / this dtype", safe_d);
  if (st == -2) {
    char size[16] = "";
    if (lds >= 0) snprintf(size, sizeof(size), "=%d", lds);
    return fail(FFPA_ERR_LAUNCH, "hipFuncSetAttribute(MaxDynamicSharedMemorySize%s) failed (is this a gfx950?)", size);
  }
  if (st < 0) return fail(FFPA_ERR_LAUNCH, "launch setup failed (%d)", st);
  return fail(FFPA_ERR_LAUNCH, "kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
}

}  // namespace

extern "C" {

int ffpa_attn_fwd(const ffpa_fwd_params* p, void* stream) {
  const DimEntry* de = nullptr;
  int rc = check_basic(p, &de, true);
  if (rc != FFPA_OK) return rc;
  if (!aligned16(p->q) || !aligned16(p->k) || !aligned16(p->v) || !aligned16(p->o))
    return fail(FFPA_ERR_MISALIGNED, "q/k/v/o base pointers must be 16-byte aligned");
  if ((rc = check_strides("q", p->q_stride, 3)) || (rc = check_strides("k", p->k_stride, 3)) ||
      (rc = check_strides("v", p->v_stride, 3)) || (rc = check_strides("o", p->o_stride, 3)))
    return rc;
  // K / V tiles are fetched with 32-bit buffer offsets relative to the tile's first row: one tile (<= 128
  // rows) must span < 4 GiB; the slice itself may be of any size
  for (const int64_t* st : {p->k_stride, p->v_stride}) {
    if (st[2] < p->head_dim || st[2] >= (1LL << 24))
      return fail(FFPA_ERR_BAD_STRIDE, "k/v row stride %lld: rows must not overlap and must be < 2^24 elements apart",
                  (long long)st[2]);
  }
  if ((p->bias == nullptr) != (p->bias_dtype == FFPA_BIAS_NONE))
    return fail(FFPA_ERR_BAD_DTYPE, "bias pointer and bias_dtype disagree (ptr %s, dtype %d)",
                p->bias ? "set" : "NULL", p->bias_dtype);
  if (p->bias_dtype < FFPA_BIAS_NONE || p->bias_dtype > FFPA_BIAS_BOOL8)
    return fail(FFPA_ERR_BAD_DTYPE, "unknown bias_dtype %d", p->bias_dtype);
  for (int i = 0; i < 4; ++i)
    if (p->bias && p->bias_stride[i] < 0) return fail(FFPA_ERR_BAD_STRIDE, "bias stride[%d] is negative", i);
  if (!(p->dropout_p >= 0.f && p->dropout_p < 1.f))
    return fail(FFPA_ERR_BAD_SHAPE, "dropout_p=%g must be in [0, 1)", (double)p->dropout_p);
  if (p->dropout_p > 0.f && p->causal_row_mod != 0)
    return fail(FFPA_ERR_UNSUPPORTED, "dropout with packed query heads (causal_row_mod) is not supported");
  if (!isfinite(p->softmax_scale)) return fail(FFPA_ERR_BAD_SHAPE, "softmax_scale is not finite");
  const int safe = (p->flags & FFPA_FLAG_DEBUG_SAFE_PATH) ? 1 : 0;

  if (p->causal_row_mod < 0) return fail(FFPA_ERR_BAD_SHAPE, "causal_row_mod must be >= 0");
  if (p->kv_bounds != nullptr && p->causal_row_mod != 0)
    return fail(FFPA_ERR_UNSUPPORTED, "kv_bounds with packed query heads (causal_row_mod) is not supported");
  if (p->kv_bounds != nullptr && (p->kv_bounds_stride[0] < 0 || p->kv_bounds_stride[1] < 0))
    return fail(FFPA_ERR_BAD_STRIDE, "kv_bounds strides must be >= 0");
  if (p->workspace != nullptr && !aligned16(p->workspace))
    return fail(FFPA_ERR_MISALIGNED, "workspace must be 16-byte aligned");
  if (p->split_tickets != nullptr && (reinterpret_cast<uintptr_t>(p->split_tickets) & 3u) != 0)
    return fail(FFPA_ERR_MISALIGNED, "split_tickets must be 4-byte aligned");
  if ((rc = check_device()) != FFPA_OK) return rc;
  const Plan pl = make_plan(p, de);
  const int64_t nqt = pl.nqt;
  const int64_t grid = (int64_t)p->batch * p->heads_q * (pl.pair ? (nqt + 1) / 2 : nqt) * pl.splits;
  if (grid > 0x7fffffffLL) return fail(FFPA_ERR_BAD_SHAPE, "grid of %lld workgroups is too large", (long long)grid);

  ffpa::FwdArgs a;
  memset(&a, 0, sizeof(a));
  a.q = p->q;
  a.k = p->k;
  a.v = p->v;
  a.o = p->o;
  a.lse = p->lse;
  a.bias = p->bias;
  for (int i = 0; i < 3; ++i) {
    a.sq[i] = p->q_stride[i];
    a.sk[i] = p->k_stride[i];
    a.sv[i] = p->v_stride[i];
    a.so[i] = p->o_stride[i];
  }
  for (int i = 0; i < 4; ++i) a.sbias[i] = p->bias ? p->bias_stride[i] : 0;
  a.B = p->batch;
  a.Hq = p->heads_q;
  a.Hkv = p->heads_kv;
  a.Nq = p->seqlen_q;
  a.Nkv = p->seqlen_kv;
  a.d_valid = p->head_dim;
  a.group = p->heads_q / p->heads_kv;
  a.nqt = (int)nqt;
  a.pair_tiles = pl.pair;
  a.total_wg = (int)grid;
  a.bias_dtype = p->bias_dtype;
  a.causal = p->causal ? 1 : 0;
  a.causal_offset = p->causal_offset;
  a.scale_log2 = p->softmax_scale * 1.4426950408889634f;  // FFPA_M_LOG2E, csrc/cuffpa/common.cuh:9-18
  a.inv_scale = 1.f;
  if (pl.m16) fold_scale(a, p->softmax_scale);
  a.thr = p->rescale_threshold < 0.f ? 8.0f : p->rescale_threshold;
  a.flags = p->flags & 0x7fffffffu;  // (bit 31 is the launch side's own: kFlagStreamKV)
  {
    // Short-query launches stream K / V with the non-temporal hint when nothing would hit in a cache anyway: every (batch, kv head) is read by ONE
    // workgroup per KV range (MHA, or query heads packed into the rows by the caller: heads_q == heads_kv) and K + V are past the 256 MiB Infinity
    // Cache (a cache of that size read every decode step IS served from it: B4 H32 Nkv 1024 D512 = 256 MiB measured - 5 % with the hint, 128 MiB - 3 %;
    // 288 MiB + 3 %, 320 MiB + 5 ... 7 %, 384 / 512 MiB + 5 ... 8 %: the line is drawn at 272 MiB).  LDS-DMA from HBM: 5.9
    // TB/s without the hint, 7.3 with it (tools/probes/hbm_read_probe.hip); decode B1 H32 Nkv 8192 D512 102.8 -> 95.6 us per step, B8 GQA 180 -> 169,
    // D = 1024 179 -> 170, 131072 keys 356 -> 335; un-packed GQA (several workgroups read the same K / V through L2) LOSES 2 ... 15 % and keeps the
    // plain form (profiles/r04_kv_stream.txt).
    const int64_t kv_bytes = 2LL * p->batch * p->heads_kv * p->seqlen_kv * p->head_dim * 2;
    bool stream = pl.variant == 1 && p->heads_q == p->heads_kv && kv_bytes >= (272LL << 20);
    if (p->flags & FFPA_FLAG_KV_STREAM) stream = pl.variant == 1;
    if (p->flags & FFPA_FLAG_NO_KV_STREAM) stream = false;
    if (stream) a.flags |= ffpa::kFlagStreamKV;
  }
  a.nsplit = pl.splits;
  a.tiles_per_split = pl.tiles_per_split;
  a.causal_row_mod = p->causal_row_mod;
  a.kv_bounds = p->kv_bounds;
  a.s_bounds[0] = p->kv_bounds ? p->kv_bounds_stride[0] : 0;
  a.s_bounds[1] = p->kv_bounds ? p->kv_bounds_stride[1] : 0;
  if (p->bias != nullptr && p->bias_stride[3] == 1) {
    // vector bias loads (16 consecutive keys per lane): W elements per load need W-element aligned base and
    // batch / head / row strides.  16-byte loads when possible (W = 8 for 16-bit, 4 for fp32), else 8-byte.
    const int esz = p->bias_dtype == FFPA_BIAS_FP32 ? 4 : p->bias_dtype == FFPA_BIAS_BOOL8 ? 1 : 2;
    for (int w : {16 / esz, esz == 1 ? 16 : 4}) {  // boolean masks: 16-byte loads or byte loads
      bool ok = (reinterpret_cast<uintptr_t>(p->bias) % (size_t)(w * esz)) == 0;
      for (int i = 0; i < 3; ++i) ok = ok && (p->bias_stride[i] % w == 0);
      if (ok) {
        a.bias_vec = w;
        break;
      }
    }
  }
  // A key bias (no row axis, unit key stride, 16-byte aligned rows, 16- or 32-bit) is cached in LDS once per workgroup when the
  // head dim's tiles leave room for a whole number of tiles' worth of it (ffpa_common.h: FwdArgs.bias_lds)
  if (!pl.m16 && p->bias != nullptr && pl.variant == 0 && pl.splits == 1 && p->seqlen_q > 1 && p->bias_stride[2] == 0 && p->bias_stride[3] == 1 &&
      p->bias_dtype >= FFPA_BIAS_FP16 && p->bias_dtype <= FFPA_BIAS_FP32 && !(p->flags & FFPA_FLAG_NO_BIAS_LDS) && !safe) {
    const int esz = p->bias_dtype == FFPA_BIAS_FP32 ? 4 : 2;
    const int64_t row_bytes = (int64_t)p->seqlen_kv * esz;
    const int64_t bytes = (int64_t)pl.nt * pl.bc * esz;
    const bool ok = reinterpret_cast<uintptr_t>(p->bias) % 16 == 0 && row_bytes % 16 == 0 && (p->bias_stride[0] * esz) % 16 == 0 &&
                    (p->bias_stride[1] * esz) % 16 == 0 && pl.lds + bytes <= 160 * 1024;
    if (ok) a.bias_lds = (int)bytes;
  }
  if (pl.m16) {
    a.bias_tile = pl.btile;
    a.bias_lds = pl.bias_lds;
    a.bias_cache_raw = pl.bias_raw;
  } else if (pl.btile) {
    a.bias_tile = 1;
    a.bias_lds = -(4 * 32 * pl.bc * 2);  // negative: LDS bytes reserved for the tile staging (no key-bias row cache)
  }
  a.dropout_p = p->dropout_p;
  a.keep_scale = p->dropout_p > 0.f ? 1.f / (1.f - p->dropout_p) : 1.f;
  a.keep_threshold = dropout_keep_threshold(p->dropout_p);
  // (prefill launches of the 16x16x32 build with at least two rounds of row tiles per head and XCD share a head between XCDs)
  a.xcd_group = pick_xcd_group(p->flags, pl.m16 && pl.splits == 1 && (int64_t)pl.nqt * (p->heads_q / p->heads_kv) >= 64, p->seqlen_kv, p->head_dim);
  a.l2_prefetch = pick_l2_prefetch(p->flags, pl.m16 && kernel_head_dim(p->head_dim) > 512);
  a.philox_seed = p->philox_seed;
  a.philox_offset = p->philox_offset;
  if (pl.splits > 1) {
    a.ws_o = static_cast<float*>(p->workspace);
    a.ws_lse = a.ws_o + (size_t)pl.splits * p->batch * p->heads_q * p->seqlen_q * kernel_head_dim(p->head_dim);
    // short-query launches with tickets: the kernel merges the partials itself (last split of a row tile to arrive).  Prefill tiles always
    // take the merge kernel: their row tiles are 64 - 128 rows, one workgroup merging a whole tile serialises what the merge kernel
    // spreads over thousands of workgroups (measured 2x slower: profiles/r03_split_merge.txt)
    a.tickets = pl.variant == 1 ? p->split_tickets : nullptr;
  }

  int st;
  if (pl.chunk > 1 || pl.tile_ranges) {
    // the packed-sequence kernel in its dense mode (no boundary arrays): this launch's FwdArgs as they are, that kernel's workgroup order — and, with KV ranges,
    // its per-row-tile ranges into the dense call's workspace rows [split, batch, head, row]
    ffpa::VarlenArgs va;
    memset(&va, 0, sizeof(va));
    va.lse_stride_h = p->seqlen_q;
    va.head_chunk = pl.chunk > 1 ? pl.chunk : 1;
    va.ws_head_rows = p->seqlen_q;
    va.ws_split_rows = (int64_t)p->batch * p->heads_q * p->seqlen_q;
    st = -3;
    for (const VarlenEntry& e : kVarlenDims)
      if (e.d == kernel_head_dim(p->head_dim)) st = e.launch(p->dtype, 0, a, va, static_cast<hipStream_t>(stream));
  } else {
    st = de->launch(p->dtype, safe, pl.wide ? 3 : pl.variant, a, static_cast<hipStream_t>(stream));
  }
  if (st == 0 && pl.splits > 1 && a.tickets == nullptr) {
    const unsigned rows = (unsigned)((int64_t)p->batch * p->heads_q * p->seqlen_q);
    st = ffpa::dispatch_dtype(p->dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      hipLaunchKernelGGL(ffpa::ffpa_fwd_merge_kernel<T>, dim3(rows, (unsigned)(p->head_dim + 255) / 256), dim3(64), 0, static_cast<hipStream_t>(stream), a, kernel_head_dim(p->head_dim));
      return (int)hipGetLastError();
    });
  }
  return launch_status(st, pl.lds, p->head_dim);
}

size_t ffpa_attn_fwd_workspace_bytes(const ffpa_fwd_params* params) {
  const DimEntry* de = nullptr;
  if (check_basic(params, &de) != FFPA_OK) return 0;
  // size for the split count the heuristic would pick with unlimited scratch
  const ffpa_fwd_params q = with_unlimited_scratch(*params);
  return make_plan(&q, de).ws_bytes;
}

size_t ffpa_attn_fwd_split_tickets(const ffpa_fwd_params* params) {
  const DimEntry* de = nullptr;
  if (check_basic(params, &de) != FFPA_OK) return 0;
  const ffpa_fwd_params q = with_unlimited_scratch(*params);
  const Plan pl = make_plan(&q, de);
  return (pl.splits > 1 && pl.variant == 1) ? (size_t)params->batch * params->heads_q * pl.nqt : 0;
}

int ffpa_attn_mask_kv_bounds(const void* bias, int bias_dtype, const int64_t bias_stride[4], int bb, int hb, int nq,
                             int nkv, int32_t* out, void* stream) {
  if (bias == nullptr || out == nullptr || bias_stride == nullptr) return fail(FFPA_ERR_NULL_POINTER, "bias / out / strides are NULL");
  if (bias_dtype < FFPA_BIAS_FP16 || bias_dtype > FFPA_BIAS_BOOL8) return fail(FFPA_ERR_BAD_DTYPE, "unknown bias_dtype %d", bias_dtype);
  if (bb <= 0 || hb <= 0 || nq <= 0 || nkv <= 0) return fail(FFPA_ERR_BAD_SHAPE, "non-positive mask dimension");
  for (int i = 0; i < 4; ++i)
    if (bias_stride[i] < 0) return fail(FFPA_ERR_BAD_STRIDE, "bias stride[%d] is negative", i);
  ffpa::MaskBoundsArgs m;
  m.bias = bias;
  for (int i = 0; i < 4; ++i) m.sb[i] = bias_stride[i];
  m.hb = hb;
  m.nq = nq;
  m.nkv = nkv;
  m.nblk = (nq + 31) / 32;
  m.words = (nkv + 31) / 32;
  if ((size_t)m.words * 4 > 60 * 1024) m.words = 0;  // the neutral-key bitmap must fit LDS (Nkv <= 491520); else no free range
  const size_t smem = (size_t)m.words * 4;
  m.out = out;
  const int64_t grid = (int64_t)bb * hb * m.nblk;
  if (grid > 0x7fffffffLL) return fail(FFPA_ERR_BAD_SHAPE, "mask of %lld row blocks is too large", (long long)grid);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int w = bias_dtype == FFPA_BIAS_FP32 ? 4 : bias_dtype == FFPA_BIAS_BOOL8 ? 16 : 8;  // elements per 16-byte load
  const bool vec = bias_stride[3] == 1 && nkv % w == 0 && reinterpret_cast<uintptr_t>(bias) % 16 == 0 &&
                   bias_stride[0] % w == 0 && bias_stride[1] % w == 0 && bias_stride[2] % w == 0;
  const dim3 g((unsigned)grid), blk(256);
  auto launch = [&](auto t) {
    using B = typename decltype(t)::type;
    if (vec) hipLaunchKernelGGL(ffpa::ffpa_mask_kv_bounds_vec_kernel<B>, g, blk, smem, st, m);
    else hipLaunchKernelGGL(ffpa::ffpa_mask_kv_bounds_kernel<B>, g, blk, smem, st, m);
  };
  if (bias_dtype == FFPA_BIAS_FP32) launch(ffpa::TypeTag<float>{});
  else if (bias_dtype == FFPA_BIAS_BOOL8) launch(ffpa::TypeTag<uint8_t>{});
  else if (bias_dtype == FFPA_BIAS_BF16) launch(ffpa::TypeTag<__bf16>{});
  else launch(ffpa::TypeTag<_Float16>{});
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FFPA_ERR_LAUNCH, "mask bounds launch failed: %s", hipGetErrorString(e));
  return FFPA_OK;
}

int ffpa_attn_fwd_plan(const ffpa_fwd_params* params, int out[4]) {
  const DimEntry* de = nullptr;
  const int rc = check_basic(params, &de);
  if (rc != FFPA_OK) return rc;
  if (out == nullptr) return fail(FFPA_ERR_NULL_POINTER, "out is NULL");
  const Plan pl = make_plan(params, de);
  out[0] = pl.variant;
  out[1] = pl.br;
  out[2] = pl.bc;
  out[3] = pl.splits;
  return FFPA_OK;
}

int ffpa_attn_fwd_kernel(const ffpa_fwd_params* params, char* buf, size_t n) {
  const DimEntry* de = nullptr;
  const int rc = check_basic(params, &de);
  if (rc != FFPA_OK) return rc;
  if (buf == nullptr || n == 0) return fail(FFPA_ERR_NULL_POINTER, "buf is NULL / empty");
  const Plan pl = make_plan(params, de);
  const char* dt = params->dtype == FFPA_DTYPE_FP16 ? "fp16" : "bf16";
  const int drop = params->dropout_p > 0.f ? 1 : 0;
  const char* merge = pl.splits > 1 ? ((params->split_tickets != nullptr && pl.variant == 1) ? " (in-launch split merge)" : " + ffpa_fwd_merge_kernel") : "";
  if (pl.wide) {
    snprintf(buf, n, "ffpa_fwd_m16w_kernel<%s, %d, RH=%d, MK=%d>%s", dt, de->d, pl.br / 64, pl.mk, merge);
  } else if (pl.tile_ranges) {
    snprintf(buf, n, "ffpa_fwd_m16_varlen_kernel<%s, %d> (dense launch, head chunks of %d, KV ranges per row tile)%s", dt, de->d, pl.chunk > 1 ? pl.chunk : 1, merge);
  } else if (pl.chunk > 1) {
    snprintf(buf, n, "ffpa_fwd_m16_varlen_kernel<%s, %d> (dense launch, head chunks of %d)", dt, de->d, pl.chunk);
  } else if (pl.m16) {
    snprintf(buf, n, "ffpa_fwd_m16_kernel<%s, %d, MK=%d, DROP=%d%s>%s", dt, de->d, pl.mk, drop, pl.pair ? ", PAIR" : "", merge);
  } else {
    const int nd = pl.variant == 1 ? ((de->d % 128 == 0) ? 4 : 2) : (de->d <= 512 ? 1 : 2);
    snprintf(buf, n, "ffpa_fwd_split_d_kernel<%s, %d, ND=%d%s%s%s>%s", dt, de->d, nd, (params->flags & FFPA_FLAG_DEBUG_SAFE_PATH) ? ", SAFE" : "",
             drop ? ", DROP" : "", pl.btile ? ", BTILE" : "", merge);
  }
  return FFPA_OK;
}

// ---- packed sequences (include/ffpa_attn.h: ffpa_varlen_fwd_params)
namespace {

struct VarlenPlan {
  const VarlenEntry* ve;
  int br, bc, nqt;
  int pack;  // > 0: decode batch under GQA — the query heads of a KV group are the rows of the tile (VarlenArgs::pack)
  int nt;    // 1: the build whose K / V pieces carry the non-temporal hint
  int splits;        // KV ranges per sequence (1 = the KV axis is not split)
  size_t ws_bytes;   // scratch the split launch uses
  int64_t grid;      // workgroups of the launch (all ranges)
  int compact;       // > 0: row-tile slots per head of the compact grid (VarlenArgs::compact_tiles)
};

// Validation shared by the launch and the queries; fills the plan.  Head dims below the first 16x16x32 instantiation run on it (columns past the
// caller's head dim read as zeros and are never stored, as in the dense call).  `paged`: the plan of the paged-KV kernel — 64-key tiles where the packed kernel
// takes 128 (D = 256 / 320), everything else the same rule.
// `mla`: the plan of the latent-cache call (ffpa_attn_varlen_mla_fwd) — the heads of a KV group are packed into rows HOWEVER MANY they are (see below).
// `kv_bytes`: bytes per cache element as the non-temporal rule prices them (1: the FP8 latent call).
int varlen_plan(const ffpa_varlen_fwd_params* p, VarlenPlan* out, bool paged = false, bool mla = false, int kv_bytes = 2) {
  if (p == nullptr) return fail(FFPA_ERR_NULL_POINTER, "params is NULL");
  if (p->struct_size != sizeof(ffpa_varlen_fwd_params) || p->abi_version != FFPA_ATTN_ABI_VERSION)
    return fail(FFPA_ERR_BAD_ABI, "ffpa_varlen_fwd_params ABI mismatch: size %u (want %zu), version %u (want %d)", p->struct_size,
                sizeof(ffpa_varlen_fwd_params), p->abi_version, FFPA_ATTN_ABI_VERSION);
  if (p->dtype != FFPA_DTYPE_BF16 && p->dtype != FFPA_DTYPE_FP16) return fail(FFPA_ERR_BAD_DTYPE, "dtype %d is not bf16(0)/fp16(1)", p->dtype);
  if (p->batch <= 0 || p->heads_q <= 0 || p->heads_kv <= 0 || p->max_seqlen_q <= 0 || p->max_seqlen_kv < 0)
    return fail(FFPA_ERR_BAD_SHAPE, "non-positive dimension: batch=%d Hq=%d Hkv=%d max_seqlen_q=%d max_seqlen_kv=%d", p->batch, p->heads_q, p->heads_kv,
                p->max_seqlen_q, p->max_seqlen_kv);
  if (p->heads_q % p->heads_kv != 0) return fail(FFPA_ERR_BAD_SHAPE, "num_heads: Hq=%d is not a multiple of Hkv=%d", p->heads_q, p->heads_kv);
  if (p->head_dim <= 0 || p->head_dim % 8 != 0 || p->head_dim > 1024)
    return fail(FFPA_ERR_BAD_HEADDIM, "headdim not support! D=%d (supported: multiples of 8 in [8, 1024])", p->head_dim);
  int dk = kernel_head_dim(p->head_dim);
  if (dk < FFPA_M16_MIN_D) dk = FFPA_M16_MIN_D;
  const VarlenEntry* ve = nullptr;
  for (const VarlenEntry& e : kVarlenDims)
    if (e.d == dk) ve = &e;
  if (ve == nullptr) return fail(FFPA_ERR_BAD_HEADDIM, "headdim not support! D=%d", p->head_dim);
  out->ve = ve;
  out->br = 128 / (dk <= 512 ? 1 : 2);
  out->bc = ffpa::m16_block_keys(dk, paged);
  // short query sequences under GQA — decode (one token per sequence), speculative decoding / multi-token prediction / small prefill chunks (a few) —: the group's
  // heads x the sequence's tokens ride in the rows of ONE tile per (sequence, KV head), head-major (VarlenArgs::pack) — the K / V stream of a group is read once, not
  // once per query head, and the tile's MFMA rows are `group` times better used.  Packed when every sequence's rows fit one tile: group x max_seqlen_q <= block rows.
  // Measured (tools/gpu_varlen_decode.py, profiles/r06_varlen_pack_tokens.txt): 16 sequences x 16 tokens, Hq 32 / Hkv 8, D 512: 2.2 -> 4.7 TB/s of K + V; 2.1 ... 5.2 x one workgroup per query head on five shapes, bit-identical.
  const int group = p->heads_q / p->heads_kv;
  out->pack = (group > 1 && (int64_t)group * p->max_seqlen_q <= out->br && !(p->flags & FFPA_FLAG_NO_PACK_GQA)) ? group : 0;
  out->nqt = out->pack ? 1 : (p->max_seqlen_q + out->br - 1) / out->br;
  if (mla && group > 1 && !(p->flags & FFPA_FLAG_NO_PACK_GQA) && (int64_t)group * p->max_seqlen_q <= 0x7fffffffLL) {
    // The latent-cache call packs a group WIDER THAN THE TILE as well: every query head of the model reads the one latent head (128 of them, 16 ... 64 per
    // tensor-parallel rank), so a sequence's group x max_seqlen_q packed rows are cut into ceil(group x max_seqlen_q / block rows) CHUNKS — the row tiles of the
    // packed rows, which the kernel's packed path walks like any row tile (row r = (head r / ntok, token r % ntok), whatever tile r falls into: a chunk boundary
    // may fall inside a head's tokens).  The chunks of a (sequence, KV head) are neighbours in the launch order (KV head, sequence, row tile: the head-chunk order
    // with chunks of one), so the second reader of a latent tile finds it in its XCD's L2: 128 heads x 1 token are two 64-row workgroups per sequence instead of 128.
    out->pack = group;
    out->nqt = (int)(((int64_t)group * p->max_seqlen_q + out->br - 1) / out->br);
  }
  out->grid = (int64_t)p->batch * (out->pack ? p->heads_kv : p->heads_q) * out->nqt;
  // The COMPACT grid: a caller that says how many rows q has (total_q, ABI 6; >= cu_seqlens_q[batch]) lets a ragged prefill batch size its grid by the rows there are —
  // sum_i ceil(len_i / block rows) <= ceil(total_q / block rows) + batch slots per head — instead of batch x the longest sequence's row tiles, most of which would find
  // no row and leave (each of them still holds a CU for a launch and a few loads).  The kernel finds a slot's (sequence, row tile) on the device — a scan every
  // workgroup pays —, so it is taken when at least three quarters of the full grid would be idle: one 16k-token prompt among 63 short ones 7454 -> 7039 us (+ 6 %),
  // 8192 + 31 short + 4 %, D = 128 one 8k among 127 short ones + 46 %; the bench batch (8 sequences of 256 ... 4864: 55 % idle) - 1 % and not taken
  // (tools/gpu_varlen_compact.py, profiles/r06_varlen_compact_grid.txt).  FFPA_FLAG_NO_COMPACT_GRID keeps the full grid (same order, same bits).
  out->compact = 0;
  if (!out->pack && out->nqt > 1 && p->total_q > 0 && !(p->flags & FFPA_FLAG_NO_COMPACT_GRID)) {
    const int64_t slots = ((int64_t)p->total_q + out->br - 1) / out->br + p->batch;
    if (slots * 4 <= (int64_t)p->batch * out->nqt && slots <= 0x7fffffffLL) {
      out->compact = (int)slots;
      out->grid = slots * p->heads_q;
    }
  }
  // The same for the PACKED rows of a ragged latent-cache batch (one 40-token verification among five decodes at 128 heads: 480 workgroups of which 91 find rows;
  // a 512-token chunk among 63 decodes: 65 536, about 1 150).  A sequence of len_b tokens has ceil(group x len_b / block rows) chunks — what the MLA build's scan
  // counts (ffpa_fwd_m16_varlen_seq.inc) —, and sum_b ceil(group x len_b / BR) <= sum_b (group x len_b / BR + 1) <= ceil(group x total_q / BR) + batch: the
  // slots per KV head.  The grid is slots x Hkv in the launch order it had (KV head, sequence, row tile): the chunks of a (sequence, latent head) stay neighbours.
  // The three-quarter threshold is the rule above carried over — FITTED ON THE UNPACKED PREFILL KERNEL, not on this one (profiles/r18_mla_varlen.md: every batch
  // the rule takes wins 2.5 ... 6.8 x against the full grid, one exactly on the threshold 2.9 x; the crossover was not located).  A uniform batch never meets it (slots >= batch x nqt there).  The split rule and the one-reader rule below run on this grid and nqt:
  // the non-temporal fetch stays a launch-wide decision, so a decode batch that holds a chunk (nqt > 1) loses it.
  if (mla && out->pack && out->nqt > 1 && p->total_q > 0 && !(p->flags & FFPA_FLAG_NO_COMPACT_GRID)) {
    const int64_t slots = ((int64_t)group * p->total_q + out->br - 1) / out->br + p->batch;
    if (slots * 4 <= (int64_t)p->batch * out->nqt && slots <= 0x7fffffffLL) {
      out->compact = (int)slots;
      out->grid = slots * p->heads_kv;
    }
  }
  // The non-temporal K / V fetch (the dense short-query launches' rule, ffpa_attn_fwd): every K / V byte is read by ONE workgroup — one row tile per (sequence,
  // head), and MHA or packed GQA rows — and the batch's K + V do not fit the 256 MiB Infinity Cache.  The launch side sees only max_seqlen_kv, not the lengths: it
  // prices a ragged batch at half of batch x max (>= 272 MiB of that).  LDS-DMA from HBM: 5.9 TB/s without the hint, 7.3 with it (profiles/r04_kv_stream.txt);
  // packed decode batches: profiles/r06_varlen.txt.  FFPA_FLAG_KV_STREAM / _NO_KV_STREAM force either.
  {
    const bool one_reader = out->nqt == 1 && (out->pack > 0 || group == 1);
    // (the latent-cache call: nqt counts the chunks of a packed group — a latent byte with two chunks has two readers —, and there is one stream, not K + V)
    const int64_t kv_bound = (mla ? 1LL : 2LL) * p->batch * p->heads_kv * (int64_t)p->max_seqlen_kv * p->head_dim * kv_bytes;
    bool nt = one_reader && kv_bound / (mla ? 1 : 2) >= (272LL << 20);
    if (p->flags & FFPA_FLAG_KV_STREAM) nt = true;
    if (p->flags & FFPA_FLAG_NO_KV_STREAM) nt = false;
    out->nt = nt ? 1 : 0;
  }
  // KV SPLITS (ABI 6).  A launch of one row tile per (sequence, head) — decode, speculative decoding, chunked prefill — splits every sequence's KV range over `splits`
  // workgroups (the sequence's own tiles / splits per range, computed on the device) + ffpa_varlen_merge_kernel.  The launch side sees max_seqlen_kv only.  Two
  // reasons, measured on packed decode batches (tools/gpu_varlen_splits.py, profiles/r06_varlen_splits.txt):
  //   (a) FILL the chip — the dense short-query launches' rule (pick_splits): one workgroup per CU for head dims >= 320 (a tile pair is 128 KiB of LDS there), else
  //       two; at least kT.min_tiles_short KV tiles of the longest sequence per range.  8 sequences x 8 KV heads = 64 workgroups: 649 -> 212 us with 4 ranges;
  //   (b) BALANCE a ragged batch — several sequences differ in length and the longest one's workgroups finish last: up to kT.varlen_balance_wgs workgroups per slot
  //       in ranges of at least kT.varlen_balance_min_tiles tiles (256 pairs x 4 ranges: 877 -> 728 us; 64 x 8: 181 us), as long as the partials stay a small
  //       fraction of the K + V bytes (64 query rows per sequence: 4 ranges 248 us, 16 ranges 293 us).
  //   (c) PREFILL launches (several row tiles per head) that leave most of the chip idle — chunked prefill of one long sequence with a few heads per GPU: 8 heads x
  //       8 row tiles are 64 workgroups — take the dense path's under-filled rule (pick_splits): fill the slots, at least kT.min_tiles_prefill KV tiles per
  //       range; under the causal flag every row tile shares out the tiles up to ITS diagonal (the kernel), and the launch side prices the average row tile
  //       (max_seqlen_kv - max_seqlen_q / 2 keys).  64 workgroups x 4 ranges: 679 -> 242 us (392 -> 1100 TFLOPS); 16 x 16: 2600 -> 231 us.
  out->splits = 1;
  out->ws_bytes = 0;
  if (p->total_q > 0 && p->workspace != nullptr && p->num_splits != 1 && !(p->flags & FFPA_FLAG_DETERMINISTIC)) {
    const int64_t cus = device_cu_count();
    const int64_t max_tiles = ((int64_t)p->max_seqlen_kv + out->bc - 1) / out->bc;
    int64_t want = 1;
    if ((p->flags & FFPA_FLAG_FORCE_SPLITS) && p->num_splits > 1) {
      want = p->num_splits < max_tiles ? p->num_splits : max_tiles;  // (sweeps and tests: exactly n, down to one tile per range)
    } else if (out->nqt > 1 && !(mla && out->pack)) {  // (the chunks of a packed latent group are a decode launch's workgroups: rule (a) / (b) on its grid)
      // (c): slots as in (a); the workgroups that find rows — the grid is sized by max_seqlen_q, a ragged batch's short sequences leave theirs at once — are at
      // least heads x ceil(total_q / block rows) (exact when the lengths are whole tiles; a range too many costs little, one too few a lot: 2 sequences of 1024 /
      // 256 rows, 8 heads: 2 ranges 361 us, 3 270, 4 277).  A causal launch that fills the slots only once and whose longest row tile walks >= 1.5 x the average
      // one (a whole prompt: 1 ... n tiles) takes two ranges: the second half of the long rows fills the slots the short ones leave (8 heads x 4096 x 4096:
      // 187 -> 168 us; D = 128: 78 -> 70).  profiles/r06_varlen_prefill_splits.txt
      const int64_t slots = (dk >= kT.short_one_per_cu_min_d ? 1 : 2) * cus;
      int64_t live = (int64_t)p->heads_q * (((int64_t)p->total_q + out->br - 1) / out->br);
      if (live > out->grid) live = out->grid;
      if (live < 1) live = 1;
      if (2 * live <= slots) want = slots / live;
      double avg_tiles = (double)max_tiles;
      if (p->causal) {
        const double mq = p->max_seqlen_q < p->max_seqlen_kv ? p->max_seqlen_q : p->max_seqlen_kv;  // (rows past the keys see none)
        avg_tiles = ((double)p->max_seqlen_kv - 0.5 * mq) / out->bc;
        if (want == 1 && live <= slots && (double)max_tiles >= 1.5 * avg_tiles) want = 2;
      }
      const int64_t cap = (int64_t)(avg_tiles / kT.min_tiles_prefill);
      if (want > cap) want = cap;
      if (want < 1) want = 1;
      if (p->num_splits > 1 && want > p->num_splits) want = p->num_splits;
      const double per_split = (double)p->heads_q * (double)p->total_q * ((double)dk + 1.0) * sizeof(float);
      if ((double)want * per_split > kT.max_auto_ws_bytes) want = (int64_t)(kT.max_auto_ws_bytes / per_split);
    } else {
      const int64_t slots = (dk >= kT.short_one_per_cu_min_d ? 1 : 2) * cus;
      int64_t fill = 2 * out->grid <= slots ? slots / out->grid : 1;
      if (fill > max_tiles / kT.min_tiles_short) fill = max_tiles / kT.min_tiles_short;
      int64_t balance = 1;
      if (p->batch > 1 && out->grid < kT.varlen_balance_wgs * slots) {
        balance = kT.varlen_balance_wgs * slots / out->grid;
        if (balance > max_tiles / kT.varlen_balance_min_tiles) balance = max_tiles / kT.varlen_balance_min_tiles;
        // partials: splits x Hq x total_q x D x 4 B, written and read back; K + V: every pair streams its sequence — priced at 0.6 x the longest (a ragged batch)
        const double kv_bytes = (double)out->grid * 0.6 * (double)p->max_seqlen_kv * dk * 4.0;
        const double per_split_rw = 2.0 * (double)p->heads_q * (double)p->total_q * dk * 4.0;
        const int64_t afford = (int64_t)(kT.varlen_partial_frac * kv_bytes / per_split_rw);
        if (balance > afford) balance = afford;
      }
      want = fill > balance ? fill : balance;
      if (want < 1) want = 1;
      if (p->num_splits > 1 && want > p->num_splits) want = p->num_splits;
    }
    if (want > ffpa::kMergeMaxSplits) want = ffpa::kMergeMaxSplits;
    const size_t per_split = (size_t)p->heads_q * (size_t)p->total_q * ((size_t)dk + 1) * sizeof(float);
    if ((uint64_t)want * per_split > p->workspace_bytes) want = (int64_t)(p->workspace_bytes / per_split);
    if (want > 1 && out->grid * want <= 0x7fffffffLL) {
      out->splits = (int)want;
      out->ws_bytes = (size_t)want * per_split;
      out->grid *= want;
    }
  }
  if (out->grid > 0x7fffffffLL) return fail(FFPA_ERR_BAD_SHAPE, "grid of %lld workgroups is too large", (long long)out->grid);
  return FFPA_OK;
}

// A page pool (ffpa_paged_kv): the paged attention call's and the KV-cache append's
int check_pool(const ffpa_paged_kv* kv) {
  if (kv->struct_size != sizeof(ffpa_paged_kv))
    return fail(FFPA_ERR_BAD_ABI, "ffpa_paged_kv ABI mismatch: size %u (want %zu)", kv->struct_size, sizeof(ffpa_paged_kv));
  if (kv->block_table == nullptr) return fail(FFPA_ERR_NULL_POINTER, "block_table must be non-NULL");
  if (reinterpret_cast<uintptr_t>(kv->block_table) & 3u) return fail(FFPA_ERR_MISALIGNED, "block_table must be 4-byte aligned");
  if (kv->page_size <= 0 || kv->page_size % 64 != 0) return fail(FFPA_ERR_BAD_SHAPE, "page_size=%d is not a positive multiple of 64", kv->page_size);
  if (kv->pages_per_row <= 0 || kv->num_pages <= 0)
    return fail(FFPA_ERR_BAD_SHAPE, "pages_per_row=%d / num_pages=%d must be positive", kv->pages_per_row, kv->num_pages);
  if ((int64_t)kv->pages_per_row * kv->page_size > 0x7fffffffLL)
    return fail(FFPA_ERR_BAD_SHAPE, "pages_per_row x page_size = %lld keys per sequence is too large", (long long)kv->pages_per_row * kv->page_size);
  if (kv->bt_stride < kv->pages_per_row)
    return fail(FFPA_ERR_BAD_STRIDE, "bt_stride=%lld is smaller than pages_per_row=%d", (long long)kv->bt_stride, kv->pages_per_row);
  for (const int64_t st : {kv->k_page_stride, kv->v_page_stride}) {
    if (st < 0) return fail(FFPA_ERR_BAD_STRIDE, "page stride %lld is negative", (long long)st);
    if (st % 8 != 0) return fail(FFPA_ERR_BAD_STRIDE, "page stride %lld is not a multiple of 8 elements (16 bytes)", (long long)st);
  }
  return FFPA_OK;
}

// The paged call's own arguments (ffpa_paged_kv), checked behind the packed call's plan and before anything touches the device.
int check_paged(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv) {
  if (kv == nullptr) return fail(FFPA_ERR_NULL_POINTER, "paged kv is NULL");
  // (the order of the checks is the paged call's: struct size, block_table, seqused_kv, then the rest of the pool)
  if (kv->struct_size == sizeof(ffpa_paged_kv) && kv->block_table != nullptr && p->seqused_kv == nullptr)
    return fail(FFPA_ERR_NULL_POINTER, "seqused_kv must be non-NULL: it gives the paged call's key lengths");
  return check_pool(kv);
}

// The tree call's own argument (ffpa_tree_mask), checked behind the packed call's plan (and the paged pool) and before anything touches the device.
int check_tree(const ffpa_varlen_fwd_params* p, const ffpa_tree_mask* tree) {
  if (tree == nullptr) return fail(FFPA_ERR_NULL_POINTER, "tree mask is NULL");
  if (tree->struct_size != sizeof(ffpa_tree_mask))
    return fail(FFPA_ERR_BAD_ABI, "ffpa_tree_mask ABI mismatch: size %u (want %zu)", tree->struct_size, sizeof(ffpa_tree_mask));
  if (tree->bits == nullptr) return fail(FFPA_ERR_NULL_POINTER, "tree mask bits must be non-NULL");
  if (reinterpret_cast<uintptr_t>(tree->bits) & 7u) return fail(FFPA_ERR_MISALIGNED, "tree mask bits must be 8-byte aligned");
  if (tree->tokens < 1 || tree->tokens > 64) return fail(FFPA_ERR_BAD_SHAPE, "tree mask tokens=%d is outside [1, 64] (one 64-bit word per token)", tree->tokens);
  if (p->max_seqlen_q > tree->tokens)
    return fail(FFPA_ERR_BAD_SHAPE, "max_seqlen_q=%d exceeds the tree mask's tokens=%d", p->max_seqlen_q, tree->tokens);
  if (tree->batch_stride != 0 && tree->batch_stride < tree->tokens)
    return fail(FFPA_ERR_BAD_STRIDE, "tree mask batch_stride=%lld is neither 0 (one tree for the batch) nor >= tokens=%d", (long long)tree->batch_stride, tree->tokens);
  return FFPA_OK;
}

// The window call's own argument (ffpa_window), checked behind the packed call's plan (and the paged pool) and before anything touches the device.
int check_window(const ffpa_window* w) {
  if (w == nullptr) return fail(FFPA_ERR_NULL_POINTER, "window is NULL");
  if (w->struct_size != sizeof(ffpa_window)) return fail(FFPA_ERR_BAD_ABI, "ffpa_window ABI mismatch: size %u (want %zu)", w->struct_size, sizeof(ffpa_window));
  if (w->reserved != 0) return fail(FFPA_ERR_BAD_ABI, "ffpa_window.reserved=%u must be 0", w->reserved);
  if (w->left < -1 || w->right < -1) return fail(FFPA_ERR_BAD_SHAPE, "window (left=%d, right=%d): each must be >= -1 (-1 = unbounded)", w->left, w->right);
  return FFPA_OK;
}

// The soft-capping call's own argument: a finite cap > 0 (0 = "off" is the Python entry's business: it forwards to the window call), checked before any device work.
int check_softcap(float softcap) {
  if (!isfinite(softcap) || !(softcap > 0.f)) return fail(FFPA_ERR_BAD_SHAPE, "softcap=%g must be finite and > 0", (double)softcap);
  return FFPA_OK;
}

// The window the soft-capping call runs under: the caller's, or — NULL — (-1, -1), whose plan and tile walk are the plain launch's.
const ffpa_window* softcap_window(const ffpa_window* w) {
  static const ffpa_window kNone = {(uint32_t)sizeof(ffpa_window), 0u, -1, -1};
  return w != nullptr ? w : &kNone;
}

// The kernel builds of the latent-cache calls: one row per (head dim, value width) pair with the launcher of every variant of FFPA_FOR_EACH_MLA_VARIANT
// (ffpa_mla.h), indexed by MlaVariantId.
using ffpa::MlaVariant;
struct MlaBuild {
  int d, dv;
  ffpa::mla_launch_fn launch[ffpa::kMlaVariantCount];
};
const MlaBuild kMlaBuilds[] = {
#define FFPA_FN(stem, tree, gather, pool, refresh, D) &ffpa::launch_##stem##_d##D,
#define FFPA_ROW(D, DV) {D, DV, {FFPA_FOR_EACH_MLA_VARIANT(FFPA_FN, D)}},
    FFPA_FOR_EACH_MLA_BUILD(FFPA_ROW)
#undef FFPA_ROW
#undef FFPA_FN
};

// The latent-cache call's own argument (ffpa_mla), checked behind the plan (and the pool) and before anything touches the device.
int check_mla(const ffpa_varlen_fwd_params* p, const ffpa_mla* m, const MlaBuild** build) {
  if (m == nullptr) return fail(FFPA_ERR_NULL_POINTER, "mla is NULL");
  if (m->struct_size != sizeof(ffpa_mla)) return fail(FFPA_ERR_BAD_ABI, "ffpa_mla ABI mismatch: size %u (want %zu)", m->struct_size, sizeof(ffpa_mla));
  if (m->reserved != 0) return fail(FFPA_ERR_BAD_ABI, "ffpa_mla.reserved=%u must be 0", m->reserved);
  if (p->head_dim % 64 != 0 || m->head_dim_v <= 0 || m->head_dim_v % 64 != 0 || m->head_dim_v > p->head_dim)
    return fail(FFPA_ERR_BAD_SHAPE, "(head_dim, head_dim_v) = (%d, %d): both must be multiples of 64 with 0 < head_dim_v <= head_dim", p->head_dim, m->head_dim_v);
  const MlaBuild* found = nullptr;
  for (const MlaBuild& e : kMlaBuilds)
    if (e.d == p->head_dim && e.dv == m->head_dim_v) found = &e;
  if (found == nullptr) return fail(FFPA_ERR_BAD_HEADDIM, "(head_dim, head_dim_v) = (%d, %d) is not built (built: (576, 512))", p->head_dim, m->head_dim_v);
  if (m->seqlen_new < 0) return fail(FFPA_ERR_BAD_SHAPE, "ffpa_mla.seqlen_new=%d must not be negative", m->seqlen_new);
  if (m->seqlen_new > 0) {
    if (m->kv_new == nullptr || m->cache_seqlens == nullptr) return fail(FFPA_ERR_NULL_POINTER, "kv_new / cache_seqlens must be non-NULL when seqlen_new > 0");
    if (!aligned16(m->kv_new) || (reinterpret_cast<uintptr_t>(m->cache_seqlens) & 3u))
      return fail(FFPA_ERR_MISALIGNED, "kv_new must be 16-byte aligned and cache_seqlens 4-byte aligned");
    if (m->cache_seqlens == p->seqused_kv) return fail(FFPA_ERR_BAD_SHAPE, "seqused_kv receives the lengths behind the append: it must not be cache_seqlens");
    const int rc = check_strides("kv_new", m->kv_new_stride, 3);
    if (rc != FFPA_OK) return rc;
    if ((int64_t)p->batch * m->seqlen_new > 0x7fffffffLL) return fail(FFPA_ERR_BAD_SHAPE, "grid of %lld new rows is too large", (long long)p->batch * m->seqlen_new);
  }
  *build = found;
  return FFPA_OK;
}

// The FP8 latent call's own argument (ffpa_mla_fp8): its struct, checked in front of everything else of the call ...
int check_mla_fp8(const ffpa_mla_fp8* f8) {
  if (f8 == nullptr) return fail(FFPA_ERR_NULL_POINTER, "mla_fp8 is NULL");
  if (f8->struct_size != sizeof(ffpa_mla_fp8)) return fail(FFPA_ERR_BAD_ABI, "ffpa_mla_fp8 ABI mismatch: size %u (want %zu)", f8->struct_size, sizeof(ffpa_mla_fp8));
  if (f8->reserved != 0 || f8->reserved2 != 0.f)
    return fail(FFPA_ERR_BAD_ABI, "ffpa_mla_fp8.reserved=%u / reserved2=%g must be 0", f8->reserved, (double)f8->reserved2);
  if (!isfinite(f8->kv_scale) || !(f8->kv_scale > 0.f)) return fail(FFPA_ERR_BAD_SHAPE, "ffpa_mla_fp8.kv_scale=%g must be finite and > 0", (double)f8->kv_scale);
  return FFPA_OK;
}

// ... and the geometry of a pool of one byte per element: the kernel's text doubles every cache stride (it was written for 16-bit elements) and its register loads
// and the append's stores are 8 bytes wide, so rows, heads and pages lie multiples of 16 elements apart.
int check_fp8_strides(int64_t row, int64_t head, int64_t page) {
  if (row % 16 != 0 || head % 16 != 0 || page % 16 != 0)
    return fail(FFPA_ERR_BAD_STRIDE, "FP8 pool strides (row %lld, head %lld, page %lld) must be multiples of 16 elements", (long long)row, (long long)head, (long long)page);
  return FFPA_OK;
}

// The sparse latent call's own argument (ffpa_mla_sparse), in two parts.  What it checks BEFORE the plan — both pointers, its struct, then the params' ABI (the plan
// is made from a copy of them: price_sparse) and the index list ...
int check_sparse(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s) {
  if (p == nullptr) return fail(FFPA_ERR_NULL_POINTER, "params is NULL");
  if (s == nullptr) return fail(FFPA_ERR_NULL_POINTER, "mla_sparse is NULL");
  if (s->struct_size != sizeof(ffpa_mla_sparse))
    return fail(FFPA_ERR_BAD_ABI, "ffpa_mla_sparse ABI mismatch: size %u (want %zu)", s->struct_size, sizeof(ffpa_mla_sparse));
  if (s->reserved != 0 || s->reserved2 != 0) return fail(FFPA_ERR_BAD_ABI, "ffpa_mla_sparse.reserved=%u / reserved2=%d must be 0", s->reserved, s->reserved2);
  if (p->struct_size != sizeof(ffpa_varlen_fwd_params) || p->abi_version != FFPA_ATTN_ABI_VERSION)
    return fail(FFPA_ERR_BAD_ABI, "ffpa_varlen_fwd_params ABI mismatch: size %u (want %zu), version %u (want %d)", p->struct_size,
                sizeof(ffpa_varlen_fwd_params), p->abi_version, FFPA_ATTN_ABI_VERSION);
  if (p->max_seqlen_q != 1) return fail(FFPA_ERR_BAD_SHAPE, "max_seqlen_q=%d: the sparse call takes one query token per index row (max_seqlen_q = 1)", p->max_seqlen_q);
  if (s->topk < 1 || s->num_rows < 1) return fail(FFPA_ERR_BAD_SHAPE, "topk=%d / num_rows=%d must be positive", s->topk, s->num_rows);
  if (s->indices == nullptr) return fail(FFPA_ERR_NULL_POINTER, "indices must be non-NULL");
  if ((reinterpret_cast<uintptr_t>(s->indices) & 3u) || (reinterpret_cast<uintptr_t>(s->topk_lens) & 3u))
    return fail(FFPA_ERR_MISALIGNED, "indices / topk_lens must be 4-byte aligned");
  if (s->indices_stride < s->topk) return fail(FFPA_ERR_BAD_STRIDE, "indices_stride=%lld is smaller than topk=%d", (long long)s->indices_stride, s->topk);
  return FFPA_OK;
}

// The reach of the sparse kernel's addressing: every lane offset is 32 bits from the head's first row and bit 31 (kDmaOob) is the "no row" sentinel, so the rows of a
// head span at most 2^31 bytes.
constexpr int64_t kSparseSpanBytes = 1LL << 31;

// ... and what it checks BEHIND the plan and the (head_dim, head_dim_v) pair: the latent pool's geometry.  `esz`: bytes per pool element (2; 1: the FP8 sparse
// call, whose span is counted in ITS bytes — the same 2^31 reach holds twice as many rows).
int check_sparse_pool(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, int esz = 2) {
  const int rc = check_strides("kv", s->kv_stride, 2);
  if (rc != FFPA_OK) return rc;
  if (s->kv_stride[0] < p->head_dim || s->kv_stride[0] >= (1LL << 24))
    return fail(FFPA_ERR_BAD_STRIDE, "kv row stride %lld: rows must not overlap and must be < 2^24 elements apart", (long long)s->kv_stride[0]);
  const int64_t span = ((int64_t)s->num_rows - 1) * s->kv_stride[0] * esz + (int64_t)p->head_dim * esz;
  if (span > kSparseSpanBytes)
    return fail(FFPA_ERR_BAD_SHAPE, "the pool's rows span %lld bytes per head: the sparse call reaches at most 2^31 = %lld ((num_rows - 1) * row stride * %d + head_dim * %d)",
                (long long)span, (long long)kSparseSpanBytes, esz, esz);
  return FFPA_OK;
}

// The geometry of a pool of 656-byte FP8 rows (ffpa_attn_varlen_mla_sparse_ds_fwd), behind the plan and the (head_dim, head_dim_v) pair, in this order: q's dtype
// (the rotary bytes of a row are bf16 and reach the kernel's image as they are), the one row format there is, the strides — in BYTES; the kernel's text doubles
// every stride and its loads are 16 bytes wide —, the base, the reach of the 32-bit offsets.
int check_sparse_ds_pool(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s) {
  if (p->dtype != FFPA_DTYPE_BF16) return fail(FFPA_ERR_BAD_DTYPE, "dtype %d: the 656-byte rows carry bf16 rotary columns, q must be bf16(0)", p->dtype);
  if (p->head_dim != ffpa::kDsNope + 64 || s->head_dim_v != ffpa::kDsNope)
    return fail(FFPA_ERR_BAD_HEADDIM, "(head_dim, head_dim_v) = (%d, %d): a 656-byte row holds (576, 512)", p->head_dim, s->head_dim_v);
  if (s->kv_stride[0] < 0 || s->kv_stride[1] < 0 || s->kv_stride[0] % 16 != 0 || s->kv_stride[1] % 16 != 0 || s->kv_stride[0] < ffpa::kDsRowBytes ||
      s->kv_stride[0] >= (1LL << 24))
    return fail(FFPA_ERR_BAD_STRIDE, "kv strides (slot %lld, head %lld) must be multiples of 16 bytes, slots at least %d and less than 2^24 bytes apart",
                (long long)s->kv_stride[0], (long long)s->kv_stride[1], ffpa::kDsRowBytes);
  if (!aligned16(p->k)) return fail(FFPA_ERR_MISALIGNED, "the pool's base must be 16-byte aligned");
  const int64_t span = ((int64_t)s->num_rows - 1) * s->kv_stride[0] + ffpa::kDsRowBytes;
  if (span > kSparseSpanBytes)
    return fail(FFPA_ERR_BAD_SHAPE, "the pool's rows span %lld bytes per head: the sparse call reaches at most 2^31 = %lld ((num_rows - 1) * slot stride + %d)",
                (long long)span, (long long)kSparseSpanBytes, ffpa::kDsRowBytes);
  return FFPA_OK;
}

// ---- The host layer of the packed call and its relatives: a call is DESCRIBED (VarlenCall), PLANNED (plan_call -> CallPlan) and LAUNCHED from its plan
// (varlen_launch); the plan / kernel / workspace / compact-slots queries are the first two steps and a read-out.
//
// What the caller passed, and WHICH call it is.  The tag says the family, never a NULL pointer: a family that needs a struct reports its absence (check_paged,
// check_tree, check_window, check_mla, check_sparse), it does not turn into another call.
enum class Family {
  kPacked,   // ffpa_attn_varlen_fwd: cu_seqlens over contiguous K / V
  kPaged,    // ffpa_attn_varlen_paged_fwd: kv (required) — k / v are page pools, the lengths are seqused_kv's, cu_seqlens_kv is not read
  kTree,     // ffpa_attn_varlen_tree_fwd: tree; kv optional (NULL: contiguous caches) — the causal launch's plan and tile walk, the *_tree_kernel builds
  kWindow,   // ffpa_attn_varlen_window_fwd: win; kv optional — the window's own plan, the *_window_kernel builds
  kSoftcap,  // ffpa_attn_varlen_softcap_fwd: softcap; win optional (NULL: (-1, -1)), kv optional — a window launch with capped scores, the *_softcap_kernel builds
  kLatent,   // the seven ffpa_attn_varlen_mla*_fwd calls: ONE pool — k is the latent pool and serves as v too (p->v is not read) —, every group packed into rows.
             // WHICH of them is VarlenCall::variant, a row of ffpa_mla.h's list: its traits say which structs the call takes (tree: tree; gather: sparse, else kv +
             // mla — with the append in front —; an e4m3 pool: fp8) and plan_latent reads nothing else of it
};
bool is_window(Family f) { return f == Family::kWindow || f == Family::kSoftcap; }

struct VarlenCall {
  Family family;
  const ffpa_varlen_fwd_params* p;
  const ffpa_paged_kv* kv;
  const ffpa_tree_mask* tree;
  const ffpa_window* win;
  float softcap;
  const ffpa_mla* mla;
  const ffpa_mla_sparse* sparse;
  const ffpa_mla_fp8* fp8;
  const MlaVariant* variant;  // kLatent: the call's row of ffpa::kMlaVariants
};
bool is_tree(const VarlenCall& c) { return c.family == Family::kTree || (c.variant != nullptr && c.variant->tree); }
bool is_sparse(const VarlenCall& c) { return c.variant != nullptr && c.variant->gather; }
typedef const ffpa_varlen_fwd_params* ParamsPtr;
VarlenCall make_call(Family family, ParamsPtr p, const ffpa_paged_kv* kv) {
  VarlenCall c = {};
  c.family = family, c.p = p, c.kv = kv;
  return c;
}
VarlenCall packed_call(ParamsPtr p) { return make_call(Family::kPacked, p, nullptr); }
VarlenCall paged_call(ParamsPtr p, const ffpa_paged_kv* kv) { return make_call(Family::kPaged, p, kv); }
VarlenCall tree_call(ParamsPtr p, const ffpa_paged_kv* kv, const ffpa_tree_mask* tree) {
  VarlenCall c = make_call(Family::kTree, p, kv);
  c.tree = tree;
  return c;
}
VarlenCall window_call(ParamsPtr p, const ffpa_paged_kv* kv, const ffpa_window* w) {
  VarlenCall c = make_call(Family::kWindow, p, kv);
  c.win = w;
  return c;
}
VarlenCall softcap_call(ParamsPtr p, const ffpa_paged_kv* kv, const ffpa_window* w, float softcap) {
  VarlenCall c = make_call(Family::kSoftcap, p, kv);
  c.win = w, c.softcap = softcap;
  return c;
}
// A latent call, by how its variant finds the keys — through a page table (kv, mla; tree and fp8 where the variant takes them) or through the gather's list
// (sparse; fp8 likewise).  The structs a variant does not take stay NULL.
VarlenCall latent_call(ffpa::MlaVariantId id, ParamsPtr p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree = nullptr,
                       const ffpa_mla_fp8* f8 = nullptr) {
  VarlenCall c = make_call(Family::kLatent, p, kv);
  c.mla = m, c.tree = tree, c.fp8 = f8;
  c.variant = &ffpa::kMlaVariants[id];
  return c;
}
VarlenCall gather_call(ffpa::MlaVariantId id, ParamsPtr p, const ffpa_mla_sparse* s, const ffpa_mla_fp8* f8 = nullptr) {
  VarlenCall c = make_call(Family::kLatent, p, nullptr);
  c.sparse = s, c.fp8 = f8;
  c.variant = &ffpa::kMlaVariants[id];
  return c;
}

// What plan_call makes of a call: everything the launch and the queries read.  (It points into itself: made in place, never copied.)
struct CallPlan {
  VarlenPlan pl;
  const ffpa_varlen_fwd_params* p;  // the params the launch runs under: the caller's, or `priced`
  ffpa_varlen_fwd_params priced;    // the family's copy of the caller's params (price_window, price_sparse; the tree latent call: under the causal flag)
  int win_causal, win_right, win_span;  // a window launch: it runs under the causal flag (right >= 0: `right` rides in the causal limit); VarlenArgs::win_right / win_span
  const ffpa_mla* mla;              // a latent launch: the caller's ffpa_mla or — the sparse call — `own_mla`; NULL: a launch over a K and a V cache
  ffpa_mla own_mla;
  ffpa::mla_launch_fn launch_mla;   // ... and the build of the variant's kernel it launches
  const ffpa_mla_fp8* fp8;          // a latent launch over an e4m3 pool: its scale
  bool byte_pool;                   // a latent launch over a pool counted in bytes (e4m3 codes, 656-byte rows): the kernel takes its strides in units of two
};

// The window call's plan is the packed call's, PRICED AT WHAT THE WINDOW LEAVES.  A row tile of R token rows (all max_seqlen_q tokens under GQA row packing, else
// the block rows) walks the keys from its first row's left bound to its last row's right bound — R + left + right of them, and never more than left +
// max_seqlen_q (the last key is the right bound of the last token) — so the split count ("fill the chip, then balance") and the non-temporal fetch ("K / V bytes
// with one reader, larger than the Infinity Cache") see that many keys, rounded up to a KV tile, and not the cache's capacity.  No left bound: the caller's
// max_seqlen_kv.  `left` / `right` at or past the longest sequence are the unbounded side they amount to (they reach the kernel as small ints).
// `pl`: the plan of the caller's own params (its tile rows and GQA packing do not depend on max_seqlen_kv).  The launch runs under the priced copy: the caller's params but
// for the causal flag and the length the plan saw; the kernel reads every sequence's own length.
void price_window(const ffpa_varlen_fwd_params* p, const ffpa_window* w, const VarlenPlan& pl, CallPlan* cp) {
  int64_t right = p->causal ? 0 : w->right;
  if (right > p->max_seqlen_q) right = p->max_seqlen_q;  // (the last token's position + max_seqlen_q - 1 is already the last key)
  int64_t left = w->left;
  if (left >= p->max_seqlen_kv) left = -1;  // (no position reaches that far back: positions are below max_seqlen_kv)
  cp->win_causal = right >= 0 ? 1 : 0;
  cp->win_right = right >= 0 ? (int)right : 0;
  cp->win_span = left >= 0 ? (int)(left + cp->win_right) : -1;
  cp->priced = *p;
  cp->priced.causal = cp->win_causal;
  if (left >= 0) {
    const int64_t rows = pl.pack || p->max_seqlen_q < pl.br ? p->max_seqlen_q : pl.br;
    int64_t tail = right >= 0 ? rows + right : (int64_t)p->max_seqlen_q;
    if (tail > p->max_seqlen_q) tail = p->max_seqlen_q;
    const int64_t keys = (left + tail + pl.bc - 1) / pl.bc * pl.bc;
    if (keys < p->max_seqlen_kv) cp->priced.max_seqlen_kv = (int)keys;
  }
  cp->p = &cp->priced;
}

// The sparse call's plan is the latent call's for a batch of T one-token sequences of topk keys ("fill the chip, then balance", the one-reader rule of the NT build,
// the row chunks of a group wider than the tile; a uniform batch never meets the compact grid): the caller's params as the latent launch reads them — the pool's
// strides, the counts as lengths — and an ffpa_mla of its own (head_dim_v; nothing is appended).
void price_sparse(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, CallPlan* cp) {
  cp->priced = *p;
  cp->priced.causal = 0;  // (the indexer has chosen visible keys)
  cp->priced.max_seqlen_kv = s->topk;
  cp->priced.k_stride[0] = s->kv_stride[0], cp->priced.k_stride[1] = s->kv_stride[1];
  cp->priced.seqused_kv = s->topk_lens;
  memset(&cp->own_mla, 0, sizeof(cp->own_mla));
  cp->own_mla.struct_size = (uint32_t)sizeof(ffpa_mla);
  cp->own_mla.head_dim_v = s->head_dim_v;
  cp->p = &cp->priced;
  cp->mla = &cp->own_mla;
}

// The seven latent calls are ONE order of checks, each step taken where the variant's traits ask for it (tests/golden/capi_varlen_calls.json pins the order, form
// by form).  Tree and gather both price a copy of the params: no variant has both.
#define FFPA_ROW(stem, tree, gather, ...) static_assert(!(tree && gather), "plan_latent prices ONE copy of the params");
FFPA_FOR_EACH_MLA_VARIANT(FFPA_ROW, )
#undef FFPA_ROW
int plan_latent(const VarlenCall& c, CallPlan* cp) {
  const MlaVariant& v = *c.variant;
  const bool e4m3 = v.pool == FFPA_MLA_POOL_E4M3, ds = v.pool == FFPA_MLA_POOL_DS;
  const int esz = v.pool == FFPA_MLA_POOL_16BIT ? 2 : 1;  // bytes per element of the pool: what the plan prices a key at, what the gather's span counts
  const ffpa_varlen_fwd_params* p = c.p;
  const MlaBuild* build = nullptr;
  int rc;
  // 1. an e4m3 pool: its own struct, in front of everything else of the call
  if (e4m3 && (rc = check_mla_fp8(c.fp8)) != FFPA_OK) return rc;
  // 2. the gather: its struct and the index list, then the params as the latent launch reads them — and an ffpa_mla of the call's own
  if (v.gather) {
    if ((rc = check_sparse(p, c.sparse)) != FFPA_OK) return rc;
    price_sparse(p, c.sparse, cp);
  }
  // 3. the tree: the latent call UNDER THE CAUSAL FLAG, whatever p->causal says (the tree launch walks the causal launch's tiles)
  if (v.tree && p != nullptr && p->struct_size == sizeof(ffpa_varlen_fwd_params)) {  // (anything else: varlen_plan refuses it by name)
    cp->priced = *p;
    cp->priced.causal = 1;
    cp->p = &cp->priced;
  }
  p = cp->p;
  const ffpa_mla* mla = v.gather ? cp->mla : c.mla;
  // 4. - 7. the plan, with a key priced at the pool's bytes; the page pool; the latent struct and the (head dim, value width) pair; the mask
  if ((rc = varlen_plan(p, &cp->pl, true, true, esz)) != FFPA_OK) return rc;
  if (!v.gather && (rc = check_paged(p, c.kv)) != FFPA_OK) return rc;
  if ((rc = check_mla(p, mla, &build)) != FFPA_OK) return rc;
  if (v.tree && (rc = check_tree(p, c.tree)) != FFPA_OK) return rc;
  // 8. the gathered pool's geometry, 9. the stride rule of a pool of one-byte elements
  if (v.gather && (rc = ds ? check_sparse_ds_pool(p, c.sparse) : check_sparse_pool(p, c.sparse, esz)) != FFPA_OK) return rc;
  if (e4m3 && (rc = v.gather ? check_fp8_strides(c.sparse->kv_stride[0], c.sparse->kv_stride[1], 0)
                             : check_fp8_strides(p->k_stride[0], p->k_stride[1], c.kv->k_page_stride)) != FFPA_OK)
    return rc;
  cp->mla = mla;
  cp->fp8 = e4m3 ? c.fp8 : nullptr;
  cp->launch_mla = build->launch[c.variant - ffpa::kMlaVariants];
  cp->byte_pool = esz == 1;
  return FFPA_OK;
}

// EVERY check of a call that precedes the device, family by family and in the family's order — this is the one place where that order is written down — and the
// plan the launch and the queries read.  The words it is written in: varlen_plan (validates the params it is given and plans them; `paged`: 64-key tiles where the
// packed kernel takes 128; `mla`: every group packed into rows), check_paged, check_tree, check_window, check_softcap and — plan_latent — check_mla, check_mla_fp8,
// check_sparse / check_sparse_pool.
int plan_call(const VarlenCall& c, CallPlan* cp) {
  const ffpa_varlen_fwd_params* p = c.p;
  VarlenPlan* pl = &cp->pl;
  const bool paged = c.kv != nullptr;
  int rc;
  cp->p = p;
  cp->win_causal = cp->win_right = cp->win_span = 0;
  cp->mla = nullptr;
  cp->launch_mla = nullptr;
  cp->fp8 = nullptr;
  cp->byte_pool = false;
  switch (c.family) {
    case Family::kPacked:
      return varlen_plan(p, pl);
    case Family::kPaged:
      if ((rc = varlen_plan(p, pl, true)) != FFPA_OK) return rc;
      return check_paged(p, c.kv);
    case Family::kTree:
      if ((rc = varlen_plan(p, pl, paged)) != FFPA_OK) return rc;
      if (paged && (rc = check_paged(p, c.kv)) != FFPA_OK) return rc;
      return check_tree(p, c.tree);
    case Family::kSoftcap:  // the window call behind the cap's own check; no window = (-1, -1)
    case Family::kWindow: {
      if (c.family == Family::kSoftcap && (rc = check_softcap(c.softcap)) != FFPA_OK) return rc;
      const ffpa_window* w = c.family == Family::kSoftcap ? softcap_window(c.win) : c.win;
      if ((rc = varlen_plan(p, pl, paged)) != FFPA_OK) return rc;  // (errors are those of the caller's params; price_window reads this plan's tile)
      if (paged && (rc = check_paged(p, c.kv)) != FFPA_OK) return rc;
      if ((rc = check_window(w)) != FFPA_OK) return rc;
      price_window(p, w, *pl, cp);
      return varlen_plan(cp->p, pl, paged);
    }
    case Family::kLatent:
      return plan_latent(c, cp);
  }
  return fail(FFPA_ERR_UNSUPPORTED, "unknown call family %d", (int)c.family);
}

// What every latent append takes of its pool — the 16-bit and the quantising one, of a [B, S] and of a ragged step —: the caller adds the new rows' strides
// (s_new) and, for a [B, S] step, Snew.  `stride`: elements between two rows / heads of the pool.
ffpa::MlaAppendArgs mla_append_args(const void* kv_new, void* cache, const int* seqlens, int* used, const int64_t stride[2], const ffpa_paged_kv* kv, int B, int Hkv, int D) {
  ffpa::MlaAppendArgs a;
  memset(&a, 0, sizeof(a));
  a.kv_new = kv_new, a.cache = cache;
  a.seqlens = seqlens, a.used = used, a.table = kv->block_table;
  a.s_row = stride[0], a.s_head = stride[1], a.s_page = kv->k_page_stride, a.bt_stride = kv->bt_stride;
  a.B = B, a.Hkv = Hkv, a.D = D;
  a.cap = kv->pages_per_row * kv->page_size, a.page_size = kv->page_size, a.num_pages = kv->num_pages;
  return a;
}

// What the two K / V appends — of a [B, S] step (ffpa_kv_append_params) and of a ragged one (ffpa_kv_append_varlen_params) — check and fill alike; P is either
// struct: the fields read here have one name in both.  The exports keep their own checks between these, in the order tests/golden/capi_append_calls.json holds.
extern "C++" {  // (templates: this file's helpers stand inside the header's extern "C")
template <class P>
int check_kv_append_dims(const P* p) {
  if (p->dtype != FFPA_DTYPE_BF16 && p->dtype != FFPA_DTYPE_FP16) return fail(FFPA_ERR_BAD_DTYPE, "dtype %d is not bf16(0)/fp16(1)", p->dtype);
  if (p->batch <= 0 || p->heads_q <= 0 || p->heads_kv <= 0)
    return fail(FFPA_ERR_BAD_SHAPE, "non-positive dimension: batch=%d Hq=%d Hkv=%d", p->batch, p->heads_q, p->heads_kv);
  if (p->heads_q % p->heads_kv != 0) return fail(FFPA_ERR_BAD_SHAPE, "num_heads: Hq=%d is not a multiple of Hkv=%d", p->heads_q, p->heads_kv);
  if (p->head_dim <= 0 || p->head_dim % 8 != 0 || p->head_dim > 1024)
    return fail(FFPA_ERR_BAD_HEADDIM, "headdim not support! D=%d (supported: multiples of 8 in [8, 1024])", p->head_dim);
  return FFPA_OK;
}

// The pool (or the slab's capacity) and the rotary tables against it -> *cap, the keys a sequence can hold.
template <class P>
int check_kv_append_cache(const P* p, const ffpa_paged_kv* kv, int* cap) {
  *cap = p->capacity;
  if (kv != nullptr) {
    const int rc = check_pool(kv);
    if (rc != FFPA_OK) return rc;
    *cap = kv->pages_per_row * kv->page_size;
  } else if (*cap <= 0) {
    return fail(FFPA_ERR_BAD_SHAPE, "capacity=%d of the contiguous cache must be positive", *cap);
  }
  const int rd = p->rotary_dim;
  if (rd < 0 || rd % 16 != 0 || rd > p->head_dim)
    return fail(FFPA_ERR_BAD_SHAPE, "rotary_dim=%d must be a multiple of 16 in [0, head_dim=%d]", rd, p->head_dim);
  if (rd > 0 && p->seqlen_ro < *cap) return fail(FFPA_ERR_BAD_SHAPE, "seqlen_ro=%d rows of rotary_cos / rotary_sin is less than the capacity %d", p->seqlen_ro, *cap);
  return FFPA_OK;
}

// Base pointers and strides of what the launch reads: the caches always, k / v, q / q_rot and the tables where it uses them; `n`: the strides of a row tensor.
template <class P>
int check_kv_append_layout(const P* p, bool use_kv, bool use_q, bool use_rot, int n) {
  if (!aligned16(p->k_cache) || !aligned16(p->v_cache) || (use_kv && (!aligned16(p->k) || !aligned16(p->v))) ||
      (use_q && (!aligned16(p->q) || !aligned16(p->q_rot))) || (use_rot && (!aligned16(p->rotary_cos) || !aligned16(p->rotary_sin))))
    return fail(FFPA_ERR_MISALIGNED, "q / k / v / caches / q_rot / rotary_cos / rotary_sin base pointers must be 16-byte aligned");
  int rc;
  if ((rc = check_strides("k_cache", p->k_cache_stride, 3)) || (rc = check_strides("v_cache", p->v_cache_stride, 3))) return rc;
  if (use_kv && ((rc = check_strides("k", p->k_stride, n)) || (rc = check_strides("v", p->v_stride, n)))) return rc;
  if (use_q && ((rc = check_strides("q", p->q_stride, n)) || (rc = check_strides("q_rot", p->q_rot_stride, n)))) return rc;
  return FFPA_OK;
}

// Everything of KvAppendArgs but the token rows' own (their strides, Sq / Snew, T), and the workgroups per token row of a grid of `grid_rows` token rows.
template <class P>
unsigned fill_kv_append(ffpa::KvAppendArgs& a, const P* p, const ffpa_paged_kv* kv, int cap, int64_t grid_rows, bool* interleaved) {
  a.q = p->q, a.k = p->k, a.v = p->v;
  a.kc = p->k_cache, a.vc = p->v_cache, a.q_rot = p->q_rot;
  a.used = p->seqused, a.seqlens = p->cache_seqlens;
  a.cos = p->rotary_cos, a.sin = p->rotary_sin;
  a.skc[0] = p->k_cache_stride[1], a.skc[1] = p->k_cache_stride[2];
  a.svc[0] = p->v_cache_stride[1], a.svc[1] = p->v_cache_stride[2];
  if (kv != nullptr) {
    a.table = kv->block_table, a.bt_stride = kv->bt_stride;
    a.kc_page_stride = kv->k_page_stride, a.vc_page_stride = kv->v_page_stride;
    a.page_size = kv->page_size, a.num_pages = kv->num_pages;
  } else {
    // one page per sequence: the slab of sequence b
    a.kc_page_stride = p->k_cache_stride[0], a.vc_page_stride = p->v_cache_stride[0];
    a.page_size = cap, a.num_pages = p->batch;
  }
  const int rd = p->rotary_dim;
  a.B = p->batch, a.Hq = p->heads_q, a.Hkv = p->heads_kv, a.D = p->head_dim;
  a.cap = cap, a.seqlen_ro = p->seqlen_ro, a.rd = rd, a.causal = p->causal ? 1 : 0;
  *interleaved = rd == 0 || p->rotary_interleaved != 0;
  a.units = *interleaved ? p->head_dim / 8 : rd / 16 + (p->head_dim - rd) / 8;
  a.slots = 256 / a.units;
  const int heads = rd > 0 ? std::max(p->heads_q, p->heads_kv) : p->heads_kv;
  // workgroups per token row: as few as let a lane walk kAppendHeadsPerLane heads with one set of cos / sin registers — but a decode batch has few token
  // rows (32 x 1 token: 32 workgroups on 256 CUs at D = 512), so spread the heads over up to one per lane until the grid covers the CUs
  const int per_wg = a.slots * ffpa::kAppendHeadsPerLane;
  const int64_t fill = ((int64_t)device_cu_count() + grid_rows - 1) / grid_rows;
  return (unsigned)std::max((heads + per_wg - 1) / per_wg, (int)std::min<int64_t>((heads + a.slots - 1) / a.slots, fill));
}
}  // extern "C++"

// Plan the call, then launch the plan: the checks every family shares (in front of the device), the argument blocks, the append in front of a latent launch, the
// kernel, the merge behind a split one.
int varlen_launch(const VarlenCall& c, void* stream) {
  CallPlan cp;
  int rc = plan_call(c, &cp);
  if (rc != FFPA_OK) return rc;
  const ffpa_varlen_fwd_params* p = cp.p;
  const VarlenPlan& pl = cp.pl;
  const ffpa_paged_kv* kv = c.kv;
  const ffpa_mla* mla = cp.mla;
  const ffpa_mla_sparse* sparse = is_sparse(c) ? c.sparse : nullptr;
  const bool latent = mla != nullptr;                   // k is the one cache: it serves as v too, p->v is not read
  const bool paged = kv != nullptr || sparse != nullptr;  // the keys are found through a table: cu_seqlens_kv is not read
  if (!p->q || !p->k || (!latent && !p->v) || !p->o) return fail(FFPA_ERR_NULL_POINTER, "q/k/v/o must be non-NULL");
  if (!p->cu_seqlens_q || (!paged && !p->cu_seqlens_kv)) return fail(FFPA_ERR_NULL_POINTER, "cu_seqlens_q / cu_seqlens_kv must be non-NULL");
  if ((reinterpret_cast<uintptr_t>(p->cu_seqlens_q) & 3u) || (!paged && (reinterpret_cast<uintptr_t>(p->cu_seqlens_kv) & 3u)) || (reinterpret_cast<uintptr_t>(p->seqused_kv) & 3u))
    return fail(FFPA_ERR_MISALIGNED, "cu_seqlens_q / cu_seqlens_kv / seqused_kv must be 4-byte aligned");
  if (!aligned16(p->q) || !aligned16(p->k) || (!latent && !aligned16(p->v)) || !aligned16(p->o))
    return fail(FFPA_ERR_MISALIGNED, "q/k/v/o base pointers must be 16-byte aligned");
  if ((rc = check_strides("q", p->q_stride, 2)) || (rc = check_strides("k", p->k_stride, 2)) || (!latent && (rc = check_strides("v", p->v_stride, 2))) ||
      (rc = check_strides("o", p->o_stride, 2)))
    return rc;
  for (const int64_t* st : {p->k_stride, latent ? p->k_stride : p->v_stride}) {
    if (st[0] < p->head_dim || st[0] >= (1LL << 24))
      return fail(FFPA_ERR_BAD_STRIDE, "k/v row stride %lld: rows must not overlap and must be < 2^24 elements apart", (long long)st[0]);
  }
  if (p->lse != nullptr && p->lse_stride_head < 0) return fail(FFPA_ERR_BAD_STRIDE, "lse_stride_head is negative");
  if (!isfinite(p->softmax_scale)) return fail(FFPA_ERR_BAD_SHAPE, "softmax_scale is not finite");
  // (the FP8 latent launch: the scores are (softmax_scale x kv_scale) q.K8 — the factor rides in the scale, no element is touched)
  const float score_scale = cp.fp8 != nullptr ? p->softmax_scale * cp.fp8->kv_scale : p->softmax_scale;
  if (!isfinite(score_scale)) return fail(FFPA_ERR_BAD_SHAPE, "softmax_scale x kv_scale is not finite");
  if (p->total_q < 0) return fail(FFPA_ERR_BAD_SHAPE, "total_q=%d is negative", p->total_q);
  if (p->workspace != nullptr && !aligned16(p->workspace)) return fail(FFPA_ERR_MISALIGNED, "workspace must be 16-byte aligned");
  if ((rc = check_device()) != FFPA_OK) return rc;

  ffpa::FwdArgs a;
  memset(&a, 0, sizeof(a));
  a.q = p->q;
  a.k = p->k;
  a.v = latent ? p->k : p->v;
  a.o = p->o;
  a.lse = p->lse;
  // element strides batch / head / row: a sequence's base is its row offset (the kernel adds it), so the batch stride is zero
  a.sq[1] = p->q_stride[1], a.sq[2] = p->q_stride[0];
  a.sk[1] = p->k_stride[1], a.sk[2] = p->k_stride[0];
  a.sv[1] = (latent ? p->k_stride : p->v_stride)[1], a.sv[2] = (latent ? p->k_stride : p->v_stride)[0];
  a.so[1] = p->o_stride[1], a.so[2] = p->o_stride[0];
  a.B = p->batch;
  a.Hq = p->heads_q;
  a.Hkv = p->heads_kv;
  a.Nq = p->max_seqlen_q;   // (the kernel replaces both by the sequence's own)
  a.Nkv = p->max_seqlen_kv;
  a.d_valid = p->head_dim;
  a.group = p->heads_q / p->heads_kv;
  a.nqt = pl.nqt;
  a.total_wg = (int)pl.grid;
  a.causal = p->causal ? 1 : 0;
  a.inv_scale = 1.f;
  fold_scale(a, score_scale);
  a.thr = p->rescale_threshold < 0.f ? 8.0f : p->rescale_threshold;
  a.flags = p->flags & (FFPA_FLAG_NO_XCD_REMAP);
  a.nsplit = 1;
  a.tiles_per_split = 0x7fffffff / 2;  // (never the binding limit: the KV axis is not split)
  a.keep_scale = 1.f;
  // (the row tiles of a packed latent group are a decode launch's workgroups, not the rounds of a prefill head: one XCD per head)
  a.xcd_group = pick_xcd_group(p->flags, !latent && (int64_t)pl.nqt * (p->heads_q / p->heads_kv) >= 64, p->max_seqlen_kv, p->head_dim);
  a.l2_prefetch = pick_l2_prefetch(p->flags, pl.ve->d > 512);

  ffpa::VarlenArgs va;
  memset(&va, 0, sizeof(va));
  va.cu_q = p->cu_seqlens_q;
  va.cu_k = paged ? nullptr : p->cu_seqlens_kv;
  va.lse_stride_h = p->lse_stride_head;
  // heads of one KV group that walk a sequence side by side (ffpa_fwd_m16_varlen_kernel; pick_head_chunk: whole chunks per XCD, never across KV groups — MHA and
  // head counts that do not divide into eight chunks run plain head-major order)
  va.head_chunk = pick_head_chunk(p->heads_q, p->heads_q / p->heads_kv);
  va.pack = pl.pack;
  va.used_k = p->seqused_kv;
  va.q_tok_stride = p->q_stride[0];
  va.o_tok_stride = p->o_stride[0];
  if (pl.pack) {
    // FwdArgs describes Hkv heads of `pack` rows: head stride = one KV group, row stride = one query head
    a.Hq = p->heads_kv;
    a.group = 1;
    a.sq[1] = p->q_stride[1] * pl.pack, a.sq[2] = p->q_stride[1];
    a.so[1] = p->o_stride[1] * pl.pack, a.so[2] = p->o_stride[1];
    if (p->max_seqlen_q == 1) a.causal = 0;  // (a single token sees every key of its sequence; more tokens: the kernel sets causal_row_mod per sequence)
    va.head_chunk = 1;  // (the rows of a tile ARE the group: KV heads share nothing)
  }
  if (is_tree(c)) {
    // the causal launch's walk with causal_offset = Nkv_i - ntok_i (the kernel, per sequence): the last token's limit is the last key, so every tile is walked and
    // the KV ranges share out all of them; one token per sequence keeps the flag here — its word may hide its own key
    a.causal = 1;
    va.tree_bits = c.tree->bits;
    va.tree_stride = c.tree->batch_stride;
    va.tree_tokens = c.tree->tokens;
  }
  if (is_window(c.family)) {
    // the causal flag as the window says (right >= 0), one packed token per sequence included: its limit is the last key either way, its LEFT bound stays
    a.causal = cp.win_causal;
    va.window = 1;
    va.win_right = cp.win_right;
    va.win_span = cp.win_span;
  }
  if (c.family == Family::kSoftcap) {
    // score = cap * tanh(|scale| q.k / cap) (the sign of the scale went into Q, a zero scale zeroes Q: fold_scale): the kernel multiplies the raw score by
    // softcap_in inside the tanh, and everything behind it — row max, exponent FMA, LSE — takes cap * log2(e) where it took scale * log2(e)
    va.softcap_in = a.q_mode == 1 ? 1.f / c.softcap : fabsf(p->softmax_scale) / c.softcap;
    a.scale_log2 = c.softcap * 1.4426950408889634f;
  }

  va.compact_tiles = pl.compact;
  va.ws_head_rows = va.ws_split_rows = 0;
  if (pl.splits > 1) {
    // partials [split, query head, token, Dk] fp32 + their LSE [split, query head, token]; the kernel finds a range's tiles from its sequence's own length
    a.nsplit = pl.splits;
    a.ws_o = static_cast<float*>(p->workspace);
    a.ws_lse = a.ws_o + (size_t)pl.splits * p->heads_q * p->total_q * pl.ve->d;
    va.ws_head_rows = p->total_q;
    va.ws_split_rows = (int64_t)p->heads_q * p->total_q;
  }

  int st;
  if (paged) {
    ffpa::PagedArgs pa;
    if (sparse != nullptr) {
      // a token's "block table" is its index row, its "pages" are single rows of the pool (the gather: ffpa_mla_variant.inc)
      memset(&pa, 0, sizeof(pa));
      pa.table = sparse->indices;
      pa.bt_stride = sparse->indices_stride;
      pa.cap = sparse->topk;
      pa.page_size = 1;
      pa.num_pages = sparse->num_rows;
    } else {
      pa.table = kv->block_table;
      pa.bt_stride = kv->bt_stride;
      pa.k_page_stride = kv->k_page_stride;
      pa.v_page_stride = latent ? kv->k_page_stride : kv->v_page_stride;
      pa.cap = kv->pages_per_row * kv->page_size;
      pa.page_size = kv->page_size;
      pa.tiles_per_page = kv->page_size / pl.bc;
      pa.num_pages = kv->num_pages;
    }
    if (latent) {
      st = 0;
      if (mla->seqlen_new > 0) {
        // the step's latent rows first, ONE store per element (there is one cache; an e4m3 pool: quantised on their way in), and the lengths the attention launch
        // behind it reads
        ffpa::MlaFp8AppendArgs fa;
        memset(&fa, 0, sizeof(fa));
        fa.a = mla_append_args(mla->kv_new, const_cast<void*>(p->k), mla->cache_seqlens, const_cast<int*>(p->seqused_kv), p->k_stride, kv, p->batch, p->heads_kv, p->head_dim);
        for (int i = 0; i < 3; ++i) fa.a.s_new[i] = mla->kv_new_stride[i];
        fa.a.Snew = mla->seqlen_new;
        if (cp.fp8 != nullptr) fa.inv = 1.f / cp.fp8->kv_scale;
        st = cp.fp8 != nullptr ? ffpa::launch_mla_fp8_append(p->dtype, fa, static_cast<hipStream_t>(stream)) : ffpa::launch_mla_append(fa.a, static_cast<hipStream_t>(stream));
      }
      // a pool counted in bytes: the kernel's text doubles every cache stride, so it takes them in units of two bytes (multiples of 16: exact)
      if (cp.byte_pool) a.sk[1] /= 2, a.sk[2] /= 2, a.sv[1] /= 2, a.sv[2] /= 2, pa.k_page_stride /= 2, pa.v_page_stride /= 2;
      ffpa::MlaFp8Args ma;
      ma.dv = mla->head_dim_v;
      ma.kv_scale = cp.fp8 != nullptr ? cp.fp8->kv_scale : 1.f;  // (read by the kernels over an e4m3 pool alone)
      if (st == 0) st = cp.launch_mla(p->dtype, pl.nt, a, va, pa, ma, static_cast<hipStream_t>(stream));
    } else {
      st = pl.ve->paged(p->dtype, pl.nt, a, va, pa, static_cast<hipStream_t>(stream));
    }
  } else {
    st = pl.ve->launch(p->dtype, pl.nt, a, va, static_cast<hipStream_t>(stream));
  }
  if (st == 0 && pl.splits > 1) {
    // (the latent-cache call: the partials keep all D columns, the merge stores the value columns — its column bound is d_valid)
    if (latent) a.d_valid = mla->head_dim_v;
    const dim3 grid((unsigned)((int64_t)p->heads_q * p->total_q), (unsigned)(a.d_valid + 255) / 256);
    st = ffpa::dispatch_dtype(p->dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      hipLaunchKernelGGL(ffpa::ffpa_varlen_merge_kernel<T>, grid, dim3(64), 0, static_cast<hipStream_t>(stream), a, va, pl.ve->d, p->batch, p->o_stride[1]);
      return (int)hipGetLastError();
    });
  }
  return launch_status(st, -1, 0);
}

// ---- The queries of a call, one helper per kind: plan the call, check the output argument, read the plan out.
int call_plan(const VarlenCall& c, int out[5]) {
  CallPlan cp;
  const int rc = plan_call(c, &cp);
  if (rc != FFPA_OK) return rc;
  if (out == nullptr) return fail(FFPA_ERR_NULL_POINTER, "out is NULL");
  out[0] = cp.pl.nqt;
  out[1] = cp.pl.br;
  out[2] = cp.pl.bc;
  out[3] = (int)cp.pl.grid;
  out[4] = cp.pl.splits;
  return FFPA_OK;
}

// The scratch of the split count the heuristic would pick with unlimited scratch; 0 for arguments the call's plan refuses (the launch refuses them too, with the
// plan's status and message, whether or not it was handed scratch).
size_t call_workspace_bytes(VarlenCall c) {
  if (c.p == nullptr || c.p->struct_size != sizeof(ffpa_varlen_fwd_params)) return 0;
  const ffpa_varlen_fwd_params q = with_unlimited_scratch(*c.p);
  c.p = &q;
  CallPlan cp;
  return plan_call(c, &cp) == FFPA_OK ? cp.pl.ws_bytes : 0;
}

int call_kernel(const VarlenCall& c, char* buf, size_t n) {
  CallPlan cp;
  const int rc = plan_call(c, &cp);
  if (rc != FFPA_OK) return rc;
  if (buf == nullptr || n == 0) return fail(FFPA_ERR_NULL_POINTER, "buf is NULL");
  const VarlenPlan& pl = cp.pl;
  const char* nt = pl.nt ? ", NT" : "";
  const char* merge = pl.splits > 1 ? " + ffpa_varlen_merge_kernel" : "";
  if (cp.mla != nullptr) {
    // (a latent call's name is formatted from the caller's params; the sparse call — a uniform batch — has never named the compact grid)
    snprintf(buf, n, "ffpa_fwd_m16_%s_kernel<%s, %d, dv=%d%s>%s%s%s", c.variant->stem, c.p->dtype == FFPA_DTYPE_BF16 ? "bf16" : "fp16", c.p->head_dim, cp.mla->head_dim_v, nt,
             pl.pack ? (pl.nqt > 1 ? " (heads packed into rows, chunked)" : " (heads packed into rows)") : "",
             pl.compact > 0 && !is_sparse(c) ? " (compact grid)" : "", merge);
  } else {
    // (a window / soft-cap call's name is formatted from the priced params)
    const char* kind = is_tree(c) ? "_tree" : c.family == Family::kSoftcap ? "_softcap" : c.family == Family::kWindow ? "_window" : "";
    snprintf(buf, n, "ffpa_fwd_m16_%s%s_kernel<%s, %d%s>%s%s", c.kv != nullptr ? "paged" : "varlen", kind, cp.p->dtype == FFPA_DTYPE_BF16 ? "bf16" : "fp16", pl.ve->d, nt,
             pl.pack ? " (GQA heads packed into rows)" : "", merge);
  }
  return FFPA_OK;
}

int call_compact_slots(const VarlenCall& c, int* slots) {
  CallPlan cp;
  const int rc = plan_call(c, &cp);
  if (rc != FFPA_OK) return rc;
  if (slots == nullptr) return fail(FFPA_ERR_NULL_POINTER, "slots is NULL");
  *slots = cp.pl.compact;
  return FFPA_OK;
}

}  // namespace

// ---- packed sequences
int ffpa_attn_varlen_fwd(const ffpa_varlen_fwd_params* p, void* stream) { return varlen_launch(packed_call(p), stream); }
int ffpa_attn_varlen_fwd_plan(const ffpa_varlen_fwd_params* p, int out[5]) { return call_plan(packed_call(p), out); }
int ffpa_attn_varlen_fwd_kernel(const ffpa_varlen_fwd_params* p, char* buf, size_t n) { return call_kernel(packed_call(p), buf, n); }
size_t ffpa_attn_varlen_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p) { return call_workspace_bytes(packed_call(p)); }

// ---- the paged-KV twin (include/ffpa_attn.h: ffpa_paged_kv)
int ffpa_attn_varlen_paged_fwd(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, void* stream) {
  if (kv == nullptr) return fail(FFPA_ERR_NULL_POINTER, "paged kv is NULL");  // (this export alone names a missing pool before anything about the params)
  return varlen_launch(paged_call(p, kv), stream);
}
int ffpa_attn_varlen_paged_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, int out[5]) { return call_plan(paged_call(p, kv), out); }
int ffpa_attn_varlen_paged_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, char* buf, size_t n) { return call_kernel(paged_call(p, kv), buf, n); }
size_t ffpa_attn_varlen_paged_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv) { return call_workspace_bytes(paged_call(p, kv)); }

// ---- the tree-mask call (include/ffpa_attn.h: ffpa_tree_mask): the packed call or its paged twin, the causal launch's plan
int ffpa_attn_varlen_tree_fwd(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_tree_mask* tree, void* stream) {
  return varlen_launch(tree_call(p, kv, tree), stream);
}
int ffpa_attn_varlen_tree_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_tree_mask* tree, int out[5]) {
  return call_plan(tree_call(p, kv, tree), out);
}
int ffpa_attn_varlen_tree_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_tree_mask* tree, char* buf, size_t n) {
  return call_kernel(tree_call(p, kv, tree), buf, n);
}
size_t ffpa_attn_varlen_tree_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_tree_mask* tree) {
  return call_workspace_bytes(tree_call(p, kv, tree));
}

// ---- the sliding-window call (include/ffpa_attn.h: ffpa_window): the packed call or its paged twin, planned at the window's length (price_window)
int ffpa_attn_varlen_window_fwd(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_window* w, void* stream) {
  return varlen_launch(window_call(p, kv, w), stream);
}
int ffpa_attn_varlen_window_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_window* w, int out[5]) {
  return call_plan(window_call(p, kv, w), out);
}
int ffpa_attn_varlen_window_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_window* w, char* buf, size_t n) {
  return call_kernel(window_call(p, kv, w), buf, n);
}
size_t ffpa_attn_varlen_window_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_window* w) {
  return call_workspace_bytes(window_call(p, kv, w));
}

// ---- the soft-capping call (include/ffpa_attn.h): the window call — its checks, its plan; w == NULL = (-1, -1) — with capped scores
int ffpa_attn_varlen_softcap_fwd(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_window* w, float softcap, void* stream) {
  return varlen_launch(softcap_call(p, kv, w, softcap), stream);
}
int ffpa_attn_varlen_softcap_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_window* w, float softcap, int out[5]) {
  return call_plan(softcap_call(p, kv, w, softcap), out);
}
int ffpa_attn_varlen_softcap_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_window* w, float softcap, char* buf, size_t n) {
  return call_kernel(softcap_call(p, kv, w, softcap), buf, n);
}
size_t ffpa_attn_varlen_softcap_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_window* w, float softcap) {
  return call_workspace_bytes(softcap_call(p, kv, w, softcap));
}

// ---- the MLA latent-cache call (include/ffpa_attn.h: ffpa_mla): the paged call on ONE pool, every group packed into rows, the append in front
int ffpa_attn_varlen_mla_fwd(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, void* stream) {
  return varlen_launch(latent_call(ffpa::kMlaVariant_mla, p, kv, m), stream);
}
int ffpa_attn_varlen_mla_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, int out[5]) {
  return call_plan(latent_call(ffpa::kMlaVariant_mla, p, kv, m), out);
}
int ffpa_attn_varlen_mla_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, char* buf, size_t n) {
  return call_kernel(latent_call(ffpa::kMlaVariant_mla, p, kv, m), buf, n);
}
size_t ffpa_attn_varlen_mla_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m) {
  return call_workspace_bytes(latent_call(ffpa::kMlaVariant_mla, p, kv, m));
}
int ffpa_attn_varlen_mla_fwd_compact_slots(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, int* slots) {
  return call_compact_slots(latent_call(ffpa::kMlaVariant_mla, p, kv, m), slots);
}

// ---- the tree-mask latent call (include/ffpa_attn.h): the latent launch under the causal flag, the element test of the draft tiles reads the mask words
int ffpa_attn_varlen_mla_tree_fwd(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree, void* stream) {
  return varlen_launch(latent_call(ffpa::kMlaVariant_mla_tree, p, kv, m, tree), stream);
}
int ffpa_attn_varlen_mla_tree_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree, int out[5]) {
  return call_plan(latent_call(ffpa::kMlaVariant_mla_tree, p, kv, m, tree), out);
}
int ffpa_attn_varlen_mla_tree_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree, char* buf, size_t n) {
  return call_kernel(latent_call(ffpa::kMlaVariant_mla_tree, p, kv, m, tree), buf, n);
}
size_t ffpa_attn_varlen_mla_tree_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree) {
  return call_workspace_bytes(latent_call(ffpa::kMlaVariant_mla_tree, p, kv, m, tree));
}
int ffpa_attn_varlen_mla_tree_fwd_compact_slots(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree, int* slots) {
  return call_compact_slots(latent_call(ffpa::kMlaVariant_mla_tree, p, kv, m, tree), slots);
}

// ---- the FP8 latent call (include/ffpa_attn.h: ffpa_mla_fp8): the latent call over a pool of e4m3 codes with one per-tensor scale
int ffpa_attn_varlen_mla_fp8_fwd(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_mla_fp8* f8, void* stream) {
  return varlen_launch(latent_call(ffpa::kMlaVariant_mla_fp8, p, kv, m, nullptr, f8), stream);
}
int ffpa_attn_varlen_mla_fp8_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_mla_fp8* f8, int out[5]) {
  return call_plan(latent_call(ffpa::kMlaVariant_mla_fp8, p, kv, m, nullptr, f8), out);
}
int ffpa_attn_varlen_mla_fp8_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_mla_fp8* f8, char* buf, size_t n) {
  return call_kernel(latent_call(ffpa::kMlaVariant_mla_fp8, p, kv, m, nullptr, f8), buf, n);
}
size_t ffpa_attn_varlen_mla_fp8_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_mla_fp8* f8) {
  return call_workspace_bytes(latent_call(ffpa::kMlaVariant_mla_fp8, p, kv, m, nullptr, f8));
}
int ffpa_attn_varlen_mla_fp8_fwd_compact_slots(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_mla_fp8* f8, int* slots) {
  return call_compact_slots(latent_call(ffpa::kMlaVariant_mla_fp8, p, kv, m, nullptr, f8), slots);
}

// ---- the FP8 tree-mask latent call: the tree-mask latent call over a pool of e4m3 codes (the FP8 latent call's plan, append and scale)
int ffpa_attn_varlen_mla_tree_fp8_fwd(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree, const ffpa_mla_fp8* f8,
                                      void* stream) {
  return varlen_launch(latent_call(ffpa::kMlaVariant_mla_tree_fp8, p, kv, m, tree, f8), stream);
}
int ffpa_attn_varlen_mla_tree_fp8_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree, const ffpa_mla_fp8* f8,
                                           int out[5]) {
  return call_plan(latent_call(ffpa::kMlaVariant_mla_tree_fp8, p, kv, m, tree, f8), out);
}
int ffpa_attn_varlen_mla_tree_fp8_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree,
                                             const ffpa_mla_fp8* f8, char* buf, size_t n) {
  return call_kernel(latent_call(ffpa::kMlaVariant_mla_tree_fp8, p, kv, m, tree, f8), buf, n);
}
size_t ffpa_attn_varlen_mla_tree_fp8_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree,
                                                         const ffpa_mla_fp8* f8) {
  return call_workspace_bytes(latent_call(ffpa::kMlaVariant_mla_tree_fp8, p, kv, m, tree, f8));
}
int ffpa_attn_varlen_mla_tree_fp8_fwd_compact_slots(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree,
                                                    const ffpa_mla_fp8* f8, int* slots) {
  return call_compact_slots(latent_call(ffpa::kMlaVariant_mla_tree_fp8, p, kv, m, tree, f8), slots);
}

// ---- the FP8 sparse latent call: the sparse latent call over a pool of e4m3 codes
int ffpa_attn_varlen_mla_sparse_fp8_fwd(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, const ffpa_mla_fp8* f8, void* stream) {
  return varlen_launch(gather_call(ffpa::kMlaVariant_mla_sparse_fp8, p, s, f8), stream);
}
int ffpa_attn_varlen_mla_sparse_fp8_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, const ffpa_mla_fp8* f8, int out[5]) {
  return call_plan(gather_call(ffpa::kMlaVariant_mla_sparse_fp8, p, s, f8), out);
}
int ffpa_attn_varlen_mla_sparse_fp8_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, const ffpa_mla_fp8* f8, char* buf, size_t n) {
  return call_kernel(gather_call(ffpa::kMlaVariant_mla_sparse_fp8, p, s, f8), buf, n);
}
size_t ffpa_attn_varlen_mla_sparse_fp8_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, const ffpa_mla_fp8* f8) {
  return call_workspace_bytes(gather_call(ffpa::kMlaVariant_mla_sparse_fp8, p, s, f8));
}

// ---- the sparse latent call over the 656-byte FP8 rows of DeepSeek-V3.2, and the store that writes such rows by slot
int ffpa_attn_varlen_mla_sparse_ds_fwd(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, void* stream) {
  return varlen_launch(gather_call(ffpa::kMlaVariant_mla_sparse_ds, p, s), stream);
}
int ffpa_attn_varlen_mla_sparse_ds_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, int out[5]) {
  return call_plan(gather_call(ffpa::kMlaVariant_mla_sparse_ds, p, s), out);
}
int ffpa_attn_varlen_mla_sparse_ds_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, char* buf, size_t n) {
  return call_kernel(gather_call(ffpa::kMlaVariant_mla_sparse_ds, p, s), buf, n);
}
size_t ffpa_attn_varlen_mla_sparse_ds_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s) {
  return call_workspace_bytes(gather_call(ffpa::kMlaVariant_mla_sparse_ds, p, s));
}
int ffpa_attn_mla_ds_store(const ffpa_mla_ds_store_params* p, void* stream) {
  if (p == nullptr) return fail(FFPA_ERR_NULL_POINTER, "params is NULL");
  if (p->struct_size != sizeof(ffpa_mla_ds_store_params))
    return fail(FFPA_ERR_BAD_ABI, "ffpa_mla_ds_store_params ABI mismatch: size %u (want %zu)", p->struct_size, sizeof(ffpa_mla_ds_store_params));
  if (p->reserved != 0 || p->reserved2 != 0) return fail(FFPA_ERR_BAD_ABI, "ffpa_mla_ds_store_params.reserved=%u / reserved2=%d must be 0", p->reserved, p->reserved2);
  if (p->dtype != FFPA_DTYPE_BF16) return fail(FFPA_ERR_BAD_DTYPE, "dtype %d: the 656-byte rows carry bf16 rotary columns, kv_new must be bf16(0)", p->dtype);
  if (p->head_dim != ffpa::kDsNope + 64) return fail(FFPA_ERR_BAD_HEADDIM, "head_dim=%d: a 656-byte row holds 576 columns", p->head_dim);
  if (p->tokens < 0 || p->heads_kv <= 0 || p->num_rows <= 0)
    return fail(FFPA_ERR_BAD_SHAPE, "tokens=%d must not be negative, heads_kv=%d / num_rows=%d must be positive", p->tokens, p->heads_kv, p->num_rows);
  if ((int64_t)p->tokens * p->heads_kv > 0x7fffffffLL) return fail(FFPA_ERR_BAD_SHAPE, "grid of %lld rows is too large", (long long)p->tokens * p->heads_kv);
  if (!p->kv_cache || (p->tokens > 0 && (!p->kv_new || !p->slots))) return fail(FFPA_ERR_NULL_POINTER, "kv_cache / kv_new / slots must be non-NULL");
  if (!aligned16(p->kv_cache) || (p->tokens > 0 && !aligned16(p->kv_new)) || (reinterpret_cast<uintptr_t>(p->slots) & 3u))
    return fail(FFPA_ERR_MISALIGNED, "kv_new / kv_cache must be 16-byte aligned and slots 4-byte aligned");
  int rc;
  if (p->tokens > 0 && (rc = check_strides("kv_new", p->kv_new_stride, 2))) return rc;
  if (p->kv_cache_stride[0] < ffpa::kDsRowBytes || p->kv_cache_stride[1] < 0 || p->kv_cache_stride[0] % 16 != 0 || p->kv_cache_stride[1] % 16 != 0)
    return fail(FFPA_ERR_BAD_STRIDE, "kv_cache strides (slot %lld, head %lld) must be multiples of 16 bytes, slots at least %d bytes apart",
                (long long)p->kv_cache_stride[0], (long long)p->kv_cache_stride[1], ffpa::kDsRowBytes);
  if ((rc = check_device()) != FFPA_OK) return rc;
  ffpa::MlaDsStoreArgs a;
  memset(&a, 0, sizeof(a));
  a.kv_new = p->kv_new, a.slots = p->slots, a.pool = p->kv_cache;
  for (int i = 0; i < 2; ++i) a.s_new[i] = p->kv_new_stride[i], a.s_pool[i] = p->kv_cache_stride[i];
  a.T = p->tokens, a.Hkv = p->heads_kv, a.num_rows = p->num_rows;
  const int st = ffpa::launch_mla_ds_store(a, static_cast<hipStream_t>(stream));
  if (st != 0) return fail(FFPA_ERR_LAUNCH, "mla ds store launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
  return FFPA_OK;
}

// ---- the launch that makes the sparse latent calls' inputs (include/ffpa_attn.h: ffpa_mla_sparse_topk_params): top-k selection and the block-table translation
int ffpa_attn_mla_sparse_topk_slots(const ffpa_mla_sparse_topk_params* p, void* stream) {
  if (p == nullptr) return fail(FFPA_ERR_NULL_POINTER, "params is NULL");
  if (p->struct_size != sizeof(ffpa_mla_sparse_topk_params))
    return fail(FFPA_ERR_BAD_ABI, "ffpa_mla_sparse_topk_params ABI mismatch: size %u (want %zu)", p->struct_size, sizeof(ffpa_mla_sparse_topk_params));
  if (p->reserved != 0 || p->reserved2 != 0)
    return fail(FFPA_ERR_BAD_ABI, "ffpa_mla_sparse_topk_params.reserved=%u / reserved2=%d must be 0", p->reserved, p->reserved2);
  if ((p->scores != nullptr) == (p->positions != nullptr))
    return fail(FFPA_ERR_NULL_POINTER, "exactly one of scores / positions must be non-NULL (%s are)", p->scores != nullptr ? "both" : "neither");
  if (p->T < 0 || p->N_or_topk < 1 || p->N_or_topk > (1 << 30) || p->topk < 1)
    return fail(FFPA_ERR_BAD_SHAPE, "T=%d must not be negative, N_or_topk=%d must lie in [1, 2^30] and topk=%d must be positive", p->T, p->N_or_topk, p->topk);
  if (p->positions != nullptr && p->topk != p->N_or_topk)
    return fail(FFPA_ERR_BAD_SHAPE, "positions: N_or_topk=%d must equal topk=%d", p->N_or_topk, p->topk);
  if (p->B < 1 || (p->cu_seqlens_q == nullptr && p->T % p->B != 0))
    return fail(FFPA_ERR_BAD_SHAPE, "B=%d must be positive and, without cu_seqlens_q, divide T=%d", p->B, p->T);
  if (p->causal != 0 && p->causal != 1) return fail(FFPA_ERR_BAD_SHAPE, "causal=%d must be 0 or 1", p->causal);
  if (p->block_table != nullptr && (p->page_size < 1 || p->W < 1))
    return fail(FFPA_ERR_BAD_SHAPE, "with a block_table page_size=%d and W=%d must be positive", p->page_size, p->W);
  if (p->row_stride < 0 || p->block_table_stride < 0 || p->indices_stride < p->topk)
    return fail(FFPA_ERR_BAD_STRIDE, "row_stride=%lld / block_table_stride=%lld must not be negative, indices_stride=%lld not smaller than topk=%d",
                (long long)p->row_stride, (long long)p->block_table_stride, (long long)p->indices_stride, p->topk);
  if (p->T == 0) return FFPA_OK;
  if (!p->cache_seqlens || !p->indices || !p->topk_lens) return fail(FFPA_ERR_NULL_POINTER, "cache_seqlens / indices / topk_lens must be non-NULL");
  for (const void* ptr : {(const void*)p->scores, (const void*)p->positions, (const void*)p->cache_seqlens, (const void*)p->cu_seqlens_q,
                          (const void*)p->block_table, (const void*)p->indices, (const void*)p->topk_lens})
    if (reinterpret_cast<uintptr_t>(ptr) & 3u) return fail(FFPA_ERR_MISALIGNED, "every pointer must be 4-byte aligned");
  int rc;
  if ((rc = check_device()) != FFPA_OK) return rc;
  ffpa::MlaSparseTopkArgs a;
  memset(&a, 0, sizeof(a));
  a.scores = p->scores, a.positions = p->positions, a.cache_seqlens = p->cache_seqlens, a.cu_seqlens_q = p->cu_seqlens_q, a.block_table = p->block_table;
  a.indices = p->indices, a.topk_lens = p->topk_lens;
  a.s_row = p->row_stride, a.s_table = p->block_table_stride, a.s_out = p->indices_stride;
  a.T = p->T, a.N = p->N_or_topk, a.topk = p->topk, a.B = p->B, a.W = p->W, a.page_size = p->page_size, a.causal = p->causal;
  const int st = ffpa::launch_mla_sparse_topk(a, static_cast<hipStream_t>(stream));
  if (st != 0) return fail(FFPA_ERR_LAUNCH, "mla sparse topk launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
  return FFPA_OK;
}

// ---- the sparse latent call (include/ffpa_attn.h: ffpa_mla_sparse): the latent launch over per-token index lists
int ffpa_attn_varlen_mla_sparse_fwd(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, void* stream) {
  return varlen_launch(gather_call(ffpa::kMlaVariant_mla_sparse, p, s), stream);
}
int ffpa_attn_varlen_mla_sparse_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, int out[5]) {
  return call_plan(gather_call(ffpa::kMlaVariant_mla_sparse, p, s), out);
}
int ffpa_attn_varlen_mla_sparse_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, char* buf, size_t n) {
  return call_kernel(gather_call(ffpa::kMlaVariant_mla_sparse, p, s), buf, n);
}
size_t ffpa_attn_varlen_mla_sparse_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s) {
  return call_workspace_bytes(gather_call(ffpa::kMlaVariant_mla_sparse, p, s));
}

// ---- the latent append of a ragged step (include/ffpa_attn.h: ffpa_mla_append_varlen_params): token rows packed by cu_seqlens_q into the ONE paged pool
// (one body for the 16-bit pool and — f8 non-NULL, checked by the caller — the FP8 pool, whose rows are quantised on their way in)
static int mla_append_varlen(const ffpa_mla_append_varlen_params* p, const ffpa_paged_kv* kv, const ffpa_mla_fp8* f8, void* stream) {
  if (p == nullptr) return fail(FFPA_ERR_NULL_POINTER, "params is NULL");
  if (p->struct_size != sizeof(ffpa_mla_append_varlen_params))
    return fail(FFPA_ERR_BAD_ABI, "ffpa_mla_append_varlen_params ABI mismatch: size %u (want %zu)", p->struct_size, sizeof(ffpa_mla_append_varlen_params));
  if (p->reserved != 0 || p->reserved2 != 0) return fail(FFPA_ERR_BAD_ABI, "ffpa_mla_append_varlen_params.reserved=%u / reserved2=%d must be 0", p->reserved, p->reserved2);
  if (p->dtype != FFPA_DTYPE_BF16 && p->dtype != FFPA_DTYPE_FP16) return fail(FFPA_ERR_BAD_DTYPE, "dtype %d is not bf16(0)/fp16(1)", p->dtype);
  if (p->batch <= 0 || p->heads_kv <= 0) return fail(FFPA_ERR_BAD_SHAPE, "non-positive dimension: batch=%d Hkv=%d", p->batch, p->heads_kv);
  if (p->head_dim <= 0 || p->head_dim % 8 != 0 || p->head_dim > 1024)
    return fail(FFPA_ERR_BAD_HEADDIM, "headdim not support! D=%d (supported: multiples of 8 in [8, 1024])", p->head_dim);
  if (p->total_q < 0) return fail(FFPA_ERR_BAD_SHAPE, "total_q=%d must not be negative", p->total_q);
  if (kv == nullptr) return fail(FFPA_ERR_NULL_POINTER, "paged kv is NULL");
  int rc;
  if ((rc = check_pool(kv)) != FFPA_OK) return rc;  // (page_size % 64 among the rest)
  if (!p->kv_cache || !p->cu_seqlens_q || !p->cache_seqlens || !p->seqused)
    return fail(FFPA_ERR_NULL_POINTER, "kv_cache / cu_seqlens_q / cache_seqlens / seqused must be non-NULL");
  if (p->total_q > 0 && !p->kv_new) return fail(FFPA_ERR_NULL_POINTER, "kv_new must be non-NULL when total_q > 0");
  if (p->seqused == p->cache_seqlens) return fail(FFPA_ERR_BAD_SHAPE, "seqused must not be cache_seqlens (the kernel reads one while it writes the other)");
  if ((reinterpret_cast<uintptr_t>(p->seqused) & 3u) || (reinterpret_cast<uintptr_t>(p->cache_seqlens) & 3u) || (reinterpret_cast<uintptr_t>(p->cu_seqlens_q) & 3u))
    return fail(FFPA_ERR_MISALIGNED, "seqused / cache_seqlens / cu_seqlens_q must be 4-byte aligned");
  if (!aligned16(p->kv_cache) || (p->total_q > 0 && !aligned16(p->kv_new))) return fail(FFPA_ERR_MISALIGNED, "kv_new / kv_cache base pointers must be 16-byte aligned");
  if ((rc = check_strides("kv_cache", p->kv_cache_stride, 2)) || (p->total_q > 0 && (rc = check_strides("kv_new", p->kv_new_stride, 2)))) return rc;
  if (f8 != nullptr && (rc = check_fp8_strides(p->kv_cache_stride[0], p->kv_cache_stride[1], kv->k_page_stride)) != FFPA_OK) return rc;
  if ((rc = check_device()) != FFPA_OK) return rc;

  ffpa::MlaFp8AppendVarlenArgs fa;
  memset(&fa, 0, sizeof(fa));
  ffpa::MlaAppendVarlenArgs& va = fa.va;
  ffpa::MlaAppendArgs& a = va.a;
  a = mla_append_args(p->kv_new, p->kv_cache, p->cache_seqlens, p->seqused, p->kv_cache_stride, kv, p->batch, p->heads_kv, p->head_dim);
  a.s_new[1] = p->kv_new_stride[0], a.s_new[2] = p->kv_new_stride[1];
  va.cu_q = p->cu_seqlens_q, va.T = p->total_q;
  if (f8 != nullptr) fa.inv = 1.f / f8->kv_scale;
  const int st = f8 != nullptr ? ffpa::launch_mla_fp8_append_varlen(p->dtype, fa, static_cast<hipStream_t>(stream))
                               : ffpa::launch_mla_append_varlen(va, static_cast<hipStream_t>(stream));
  if (st != 0) return fail(FFPA_ERR_LAUNCH, "mla append (varlen) launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
  return FFPA_OK;
}
int ffpa_attn_mla_append_varlen(const ffpa_mla_append_varlen_params* p, const ffpa_paged_kv* kv, void* stream) { return mla_append_varlen(p, kv, nullptr, stream); }
int ffpa_attn_mla_fp8_append_varlen(const ffpa_mla_append_varlen_params* p, const ffpa_paged_kv* kv, const ffpa_mla_fp8* f8, void* stream) {
  const int rc = check_mla_fp8(f8);
  return rc != FFPA_OK ? rc : mla_append_varlen(p, kv, f8, stream);
}

// ---- the KV-cache append + rotary (include/ffpa_attn.h: ffpa_kv_append_params)
int ffpa_attn_kvcache_append(const ffpa_kv_append_params* p, const ffpa_paged_kv* kv, void* stream) {
  if (p == nullptr) return fail(FFPA_ERR_NULL_POINTER, "params is NULL");
  if (p->struct_size != sizeof(ffpa_kv_append_params) || p->abi_version != FFPA_ATTN_ABI_VERSION)
    return fail(FFPA_ERR_BAD_ABI, "ffpa_kv_append_params ABI mismatch: size %u (want %zu), version %u (want %d)", p->struct_size, sizeof(ffpa_kv_append_params),
                p->abi_version, FFPA_ATTN_ABI_VERSION);
  int rc, cap;
  if ((rc = check_kv_append_dims(p)) != FFPA_OK) return rc;
  if (p->seqlen_q < 0 || p->seqlen_new < 0) return fail(FFPA_ERR_BAD_SHAPE, "seqlen_q=%d / seqlen_new=%d must not be negative", p->seqlen_q, p->seqlen_new);
  if ((rc = check_kv_append_cache(p, kv, &cap)) != FFPA_OK) return rc;
  const int rd = p->rotary_dim;
  const bool use_q = rd > 0 && p->seqlen_q > 0, use_kv = p->seqlen_new > 0;
  const bool use_rot = rd > 0 && (use_q || use_kv);  // (the tables are read for every rotated q row AND every appended K row)
  if (!p->k_cache || !p->v_cache || !p->seqused || !p->cache_seqlens)
    return fail(FFPA_ERR_NULL_POINTER, "k_cache / v_cache / seqused / cache_seqlens must be non-NULL");
  if (use_kv && (!p->k || !p->v)) return fail(FFPA_ERR_NULL_POINTER, "k / v must be non-NULL when seqlen_new > 0");
  if (use_rot && (!p->rotary_cos || !p->rotary_sin))
    return fail(FFPA_ERR_NULL_POINTER, "rotary_cos / rotary_sin must be non-NULL when rotary_dim > 0");
  if (use_q && (!p->q || !p->q_rot)) return fail(FFPA_ERR_NULL_POINTER, "q / q_rot must be non-NULL when rotary_dim > 0 and seqlen_q > 0");
  if (p->seqused == p->cache_seqlens) return fail(FFPA_ERR_BAD_SHAPE, "seqused must not be cache_seqlens (the kernel reads one while it writes the other)");
  if ((reinterpret_cast<uintptr_t>(p->seqused) & 3u) || (reinterpret_cast<uintptr_t>(p->cache_seqlens) & 3u))
    return fail(FFPA_ERR_MISALIGNED, "seqused / cache_seqlens must be 4-byte aligned");
  if ((rc = check_kv_append_layout(p, use_kv, use_q, use_rot, 3)) != FFPA_OK) return rc;
  const int rows = std::max(1, std::max(p->seqlen_new, rd > 0 ? p->seqlen_q : 0));
  if ((int64_t)p->batch * rows > 0x7fffffffLL) return fail(FFPA_ERR_BAD_SHAPE, "grid of %lld token rows is too large", (long long)p->batch * rows);
  if ((rc = check_device()) != FFPA_OK) return rc;

  ffpa::KvAppendArgs a;
  memset(&a, 0, sizeof(a));
  bool interleaved;
  const unsigned grid_y = fill_kv_append(a, p, kv, cap, (int64_t)p->batch * rows, &interleaved);
  for (int i = 0; i < 3; ++i) a.sq[i] = p->q_stride[i], a.sk[i] = p->k_stride[i], a.sv[i] = p->v_stride[i], a.sqr[i] = p->q_rot_stride[i];
  a.Sq = p->seqlen_q, a.Snew = p->seqlen_new, a.T = rows;
  const int st = ffpa::launch_kv_append(p->dtype, interleaved, a, grid_y, static_cast<hipStream_t>(stream));
  if (st != 0) return fail(FFPA_ERR_LAUNCH, "kv append launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
  return FFPA_OK;
}

// ---- the same for a ragged step: token rows packed by cu_seqlens_q, optional per-token rotary positions (include/ffpa_attn.h: ffpa_kv_append_varlen_params)
int ffpa_attn_kvcache_append_varlen(const ffpa_kv_append_varlen_params* p, const ffpa_paged_kv* kv, void* stream) {
  if (p == nullptr) return fail(FFPA_ERR_NULL_POINTER, "params is NULL");
  if (p->struct_size != sizeof(ffpa_kv_append_varlen_params) || p->abi_version != FFPA_ATTN_ABI_VERSION)
    return fail(FFPA_ERR_BAD_ABI, "ffpa_kv_append_varlen_params ABI mismatch: size %u (want %zu), version %u (want %d)", p->struct_size,
                sizeof(ffpa_kv_append_varlen_params), p->abi_version, FFPA_ATTN_ABI_VERSION);
  int rc, cap;
  if ((rc = check_kv_append_dims(p)) != FFPA_OK) return rc;
  if (p->total_q < 0) return fail(FFPA_ERR_BAD_SHAPE, "total_q=%d must not be negative", p->total_q);
  if ((rc = check_kv_append_cache(p, kv, &cap)) != FFPA_OK) return rc;
  const int rd = p->rotary_dim;
  const bool rows = p->total_q > 0, use_rot = rd > 0 && rows;
  if (!p->k_cache || !p->v_cache || !p->seqused || !p->cache_seqlens || !p->cu_seqlens_q)
    return fail(FFPA_ERR_NULL_POINTER, "k_cache / v_cache / seqused / cache_seqlens / cu_seqlens_q must be non-NULL");
  if (rows && (!p->k || !p->v)) return fail(FFPA_ERR_NULL_POINTER, "k / v must be non-NULL when total_q > 0");
  if (use_rot && (!p->rotary_cos || !p->rotary_sin))
    return fail(FFPA_ERR_NULL_POINTER, "rotary_cos / rotary_sin must be non-NULL when rotary_dim > 0");
  if (use_rot && (!p->q || !p->q_rot)) return fail(FFPA_ERR_NULL_POINTER, "q / q_rot must be non-NULL when rotary_dim > 0 and total_q > 0");
  if (p->positions != nullptr && rd == 0) return fail(FFPA_ERR_BAD_SHAPE, "positions are rotary positions: they need rotary_dim > 0");
  if (p->seqused == p->cache_seqlens) return fail(FFPA_ERR_BAD_SHAPE, "seqused must not be cache_seqlens (the kernel reads one while it writes the other)");
  if ((reinterpret_cast<uintptr_t>(p->seqused) & 3u) || (reinterpret_cast<uintptr_t>(p->cache_seqlens) & 3u) ||
      (reinterpret_cast<uintptr_t>(p->cu_seqlens_q) & 3u) || (reinterpret_cast<uintptr_t>(p->positions) & 3u))
    return fail(FFPA_ERR_MISALIGNED, "seqused / cache_seqlens / cu_seqlens_q / positions must be 4-byte aligned");
  if ((rc = check_kv_append_layout(p, rows, use_rot, use_rot, 2)) != FFPA_OK) return rc;
  if ((rc = check_device()) != FFPA_OK) return rc;

  ffpa::KvAppendVarlenArgs va;
  memset(&va, 0, sizeof(va));
  ffpa::KvAppendArgs& a = va.a;
  bool interleaved;
  const unsigned grid_y = fill_kv_append(a, p, kv, cap, std::max(1, p->total_q), &interleaved);
  va.cu_q = p->cu_seqlens_q, va.positions = p->positions;
  for (int i = 0; i < 2; ++i) a.sq[i + 1] = p->q_stride[i], a.sk[i + 1] = p->k_stride[i], a.sv[i + 1] = p->v_stride[i], a.sqr[i + 1] = p->q_rot_stride[i];
  a.T = p->total_q;
  const int st = ffpa::launch_kv_append_varlen(p->dtype, interleaved, va, grid_y, static_cast<hipStream_t>(stream));
  if (st != 0) return fail(FFPA_ERR_LAUNCH, "kv append (varlen) launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
  return FFPA_OK;
}

// ---- the merge of two attention states (include/ffpa_attn.h: ffpa_merge_states_params)
int ffpa_attn_merge_states(const ffpa_merge_states_params* p, void* stream) {
  if (p == nullptr) return fail(FFPA_ERR_NULL_POINTER, "params is NULL");
  if (p->struct_size != sizeof(ffpa_merge_states_params) || p->abi_version != FFPA_ATTN_ABI_VERSION)
    return fail(FFPA_ERR_BAD_ABI, "ffpa_merge_states_params ABI mismatch: size %u (want %zu), version %u (want %d)", p->struct_size,
                sizeof(ffpa_merge_states_params), p->abi_version, FFPA_ATTN_ABI_VERSION);
  if (p->dtype != FFPA_DTYPE_BF16 && p->dtype != FFPA_DTYPE_FP16) return fail(FFPA_ERR_BAD_DTYPE, "dtype %d is not bf16(0)/fp16(1)", p->dtype);
  if (p->tokens < 0 || p->heads < 0) return fail(FFPA_ERR_BAD_SHAPE, "tokens=%d / heads=%d must not be negative", p->tokens, p->heads);
  if (p->head_dim <= 0 || p->head_dim % 8 != 0 || p->head_dim > 1024)
    return fail(FFPA_ERR_BAD_HEADDIM, "headdim not support! D=%d (supported: multiples of 8 in [8, 1024])", p->head_dim);
  if (!p->o_a || !p->o_b || !p->o || !p->lse_a || !p->lse_b) return fail(FFPA_ERR_NULL_POINTER, "o_a / o_b / o / lse_a / lse_b must be non-NULL");
  if (!aligned16(p->o_a) || !aligned16(p->o_b) || !aligned16(p->o)) return fail(FFPA_ERR_MISALIGNED, "o_a / o_b / o base pointers must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(p->lse_a) & 3u) || (reinterpret_cast<uintptr_t>(p->lse_b) & 3u) || (reinterpret_cast<uintptr_t>(p->lse) & 3u))
    return fail(FFPA_ERR_MISALIGNED, "lse_a / lse_b / lse must be 4-byte aligned");
  int rc;
  if ((rc = check_strides("o_a", p->o_a_stride, 2)) || (rc = check_strides("o_b", p->o_b_stride, 2)) || (rc = check_strides("o", p->o_stride, 2))) return rc;
  if (p->lse_a_stride_head < 0 || p->lse_b_stride_head < 0 || (p->lse != nullptr && p->lse_stride_head < 0))
    return fail(FFPA_ERR_BAD_STRIDE, "lse head strides must not be negative (lse_a %lld, lse_b %lld, lse %lld)", (long long)p->lse_a_stride_head,
                (long long)p->lse_b_stride_head, (long long)p->lse_stride_head);
  // (the output's rows must not overlap: two lanes would store one element)
  if (p->heads > 1 && p->tokens > 1) {
    const int64_t lo = std::min(p->o_stride[0], p->o_stride[1]), hi = std::max(p->o_stride[0], p->o_stride[1]);
    const int64_t inner = lo == p->o_stride[0] ? p->tokens : p->heads;
    if (lo < p->head_dim || hi < lo * inner) return fail(FFPA_ERR_BAD_STRIDE, "o strides {%lld, %lld} overlap its rows", (long long)p->o_stride[0], (long long)p->o_stride[1]);
  } else if ((p->heads > 1 && p->o_stride[1] < p->head_dim) || (p->tokens > 1 && p->o_stride[0] < p->head_dim)) {
    return fail(FFPA_ERR_BAD_STRIDE, "o strides {%lld, %lld} overlap its rows", (long long)p->o_stride[0], (long long)p->o_stride[1]);
  }
  if (p->lse != nullptr && p->heads > 1 && p->lse_stride_head < p->tokens)
    return fail(FFPA_ERR_BAD_STRIDE, "lse head stride %lld is less than tokens=%d (its rows would overlap)", (long long)p->lse_stride_head, p->tokens);
  if (p->tokens == 0 || p->heads == 0) return FFPA_OK;
  if ((rc = check_device()) != FFPA_OK) return rc;

  ffpa::MergeStatesArgs a;
  memset(&a, 0, sizeof(a));
  a.oa = p->o_a, a.ob = p->o_b, a.o = p->o;
  a.la = p->lse_a, a.lb = p->lse_b, a.l = p->lse;
  for (int i = 0; i < 2; ++i) a.soa[i] = p->o_a_stride[i], a.sob[i] = p->o_b_stride[i], a.so[i] = p->o_stride[i];
  a.sla = p->lse_a_stride_head, a.slb = p->lse_b_stride_head, a.sl = p->lse_stride_head;
  a.T = p->tokens, a.H = p->heads, a.D = p->head_dim;
  // one 16-byte chunk per lane: 256-lane workgroups once there are chunks for one on every CU (T x H x D / 8 >= 256 x CUs), 64-lane ones below that (16 rows x
  // 32 heads at D 512 = 32768 chunks: 512 workgroups of 64 on 256 CUs instead of 128 of 256), at most 8 workgroups per CU (a grid-stride loop does the rest)
  const int64_t chunks = (int64_t)p->tokens * p->heads * (p->head_dim / 8);
  const int64_t cus = device_cu_count();
  const unsigned threads = chunks >= 256 * cus ? 256u : 64u;
  const int64_t blocks = std::min<int64_t>((chunks + threads - 1) / threads, 8 * cus);
  const int st = ffpa::launch_merge_states(p->dtype, a, (unsigned)blocks, threads, static_cast<hipStream_t>(stream));
  if (st != 0) return fail(FFPA_ERR_LAUNCH, "merge states launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
  return FFPA_OK;
}

// ---- the plan launch of a shared-prefix step over the MLA latent cache (include/ffpa_attn.h: ffpa_mla_cascade_plan_params)
int ffpa_attn_mla_cascade_plan(const ffpa_mla_cascade_plan_params* p, void* stream) {
  if (p == nullptr) return fail(FFPA_ERR_NULL_POINTER, "params is NULL");
  if (p->struct_size != sizeof(ffpa_mla_cascade_plan_params) || p->abi_version != FFPA_ATTN_ABI_VERSION)
    return fail(FFPA_ERR_BAD_ABI, "ffpa_mla_cascade_plan_params ABI mismatch: size %u (want %zu), version %u (want %d)", p->struct_size,
                sizeof(ffpa_mla_cascade_plan_params), p->abi_version, FFPA_ATTN_ABI_VERSION);
  if (!p->lens || !p->block_table) return fail(FFPA_ERR_NULL_POINTER, "lens / block_table must be non-NULL");
  if (!p->cu_q_prefix || !p->prefix_lens || !p->prefix_table || !p->suffix_table || !p->suffix_lens)
    return fail(FFPA_ERR_NULL_POINTER, "cu_q_prefix / prefix_lens / prefix_table / suffix_table / suffix_lens must be non-NULL");
  if (p->batch < 1 || p->pages_per_seq < 1) return fail(FFPA_ERR_BAD_SHAPE, "batch=%d / pages_per_seq=%d must be at least 1", p->batch, p->pages_per_seq);
  if (p->groups < 1) return fail(FFPA_ERR_BAD_SHAPE, "groups=%d must be at least 1", p->groups);
  if (p->cu_group_seqs == nullptr && p->groups != 1) return fail(FFPA_ERR_BAD_SHAPE, "groups=%d without cu_group_seqs (NULL means one group)", p->groups);
  if (p->seqlen_q < 1 || (int64_t)p->batch * p->seqlen_q > INT32_MAX)
    return fail(FFPA_ERR_BAD_SHAPE, "seqlen_q=%d must be at least 1 with batch * seqlen_q < 2^31", p->seqlen_q);
  if (p->page_size <= 0 || p->page_size % 64 != 0) return fail(FFPA_ERR_BAD_SHAPE, "page_size=%d must be a positive multiple of 64", p->page_size);
  if (p->causal != 0 && p->causal != 1) return fail(FFPA_ERR_BAD_SHAPE, "causal=%d must be 0 or 1", p->causal);
  if (p->capacity <= 0 || (int64_t)p->capacity > (int64_t)p->pages_per_seq * p->page_size)
    return fail(FFPA_ERR_BAD_SHAPE, "capacity=%d must lie in (0, pages_per_seq * page_size = %lld]", p->capacity, (long long)p->pages_per_seq * p->page_size);
  if (p->shared_prefix_len == nullptr && p->shared_prefix_len_host < 0)
    return fail(FFPA_ERR_BAD_SHAPE, "shared_prefix_len_host=%d must not be negative", p->shared_prefix_len_host);
  if (p->batch > 1 && p->bt_stride < p->pages_per_seq)
    return fail(FFPA_ERR_BAD_STRIDE, "block_table row stride %lld is less than pages_per_seq=%d", (long long)p->bt_stride, p->pages_per_seq);
  // every array as a byte range: all 4-byte aligned, no output on an input or on another output (two workgroups would race, or a read would see a store)
  struct Range {
    const char* name;
    uintptr_t lo, hi;
    bool out;
  };
  const auto range = [](const char* name, const void* ptr, int64_t n, bool out) {
    return Range{name, reinterpret_cast<uintptr_t>(ptr), reinterpret_cast<uintptr_t>(ptr) + (uintptr_t)n * 4u, out};
  };
  const int64_t B = p->batch, G = p->groups, W = p->pages_per_seq;
  const Range rs[] = {
      range("cu_group_seqs", p->cu_group_seqs, p->cu_group_seqs ? G + 1 : 0, false),
      range("shared_prefix_len", p->shared_prefix_len, p->shared_prefix_len ? G : 0, false),
      range("lens", p->lens, B, false),
      range("block_table", p->block_table, (B - 1) * p->bt_stride + W, false),
      range("cu_q_prefix", p->cu_q_prefix, G + 1, true),
      range("prefix_lens", p->prefix_lens, G, true),
      range("prefix_table", p->prefix_table, G * W, true),
      range("suffix_table", p->suffix_table, B * W, true),
      range("suffix_lens", p->suffix_lens, B, true),
  };
  const int n = (int)(sizeof(rs) / sizeof(rs[0]));
  for (int i = 0; i < n; ++i)
    if (rs[i].lo & 3u) return fail(FFPA_ERR_MISALIGNED, "%s must be 4-byte aligned", rs[i].name);
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      if ((rs[i].out || rs[j].out) && rs[i].lo < rs[j].hi && rs[j].lo < rs[i].hi)
        return fail(FFPA_ERR_BAD_SHAPE, "%s overlaps %s: the outputs must overlap neither the inputs nor one another", rs[j].name, rs[i].name);
  int rc;
  if ((rc = check_device()) != FFPA_OK) return rc;

  ffpa::MlaCascadePlanArgs a;
  memset(&a, 0, sizeof(a));
  a.cu_group = p->cu_group_seqs, a.prefix = p->shared_prefix_len, a.lens = p->lens, a.table = p->block_table;
  a.cu_q_prefix = p->cu_q_prefix, a.prefix_lens = p->prefix_lens, a.prefix_table = p->prefix_table;
  a.suffix_table = p->suffix_table, a.suffix_lens = p->suffix_lens;
  a.bt_stride = p->bt_stride;
  a.B = p->batch, a.G = p->groups, a.W = p->pages_per_seq, a.page = p->page_size, a.Sq = p->seqlen_q, a.causal = p->causal;
  a.capacity = p->capacity, a.prefix_host = p->shared_prefix_len_host;
  const int st = ffpa::launch_mla_cascade_plan(a, static_cast<hipStream_t>(stream));
  if (st != 0) return fail(FFPA_ERR_LAUNCH, "mla cascade plan launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
  return FFPA_OK;
}

int ffpa_attn_query(int what) {
  switch (what) {
    case FFPA_QUERY_ABI_VERSION: return FFPA_ATTN_ABI_VERSION;
    case FFPA_QUERY_FWD_AVAILABLE: return 1;
    case FFPA_QUERY_MIN_HEAD_DIM: return 8;
    case FFPA_QUERY_MAX_HEAD_DIM: return 1024;
    case FFPA_QUERY_HEAD_DIM_MULTIPLE: return 8;
    case FFPA_QUERY_FP16_AVAILABLE: return 1;
    case FFPA_QUERY_DROPOUT_AVAILABLE: return 1;
#ifdef FFPA_INST_SAFE
    case FFPA_QUERY_DEBUG_KERNELS: return 1;  // the test-only twin library
#else
    case FFPA_QUERY_DEBUG_KERNELS: return 0;
#endif
    // what the launch plan's pricing reads from the current device (fallbacks without one): compute units, engine clock, HBM peak
    case FFPA_QUERY_DEVICE_CUS: return device_cu_count();
    case FFPA_QUERY_DEVICE_CLOCK_MHZ: return (int)(device_rates().cu_flops / 4096.0 / 1e6);
    case FFPA_QUERY_DEVICE_HBM_GBPS: return (int)(device_rates().hbm_bytes / 1e9);
    case FFPA_QUERY_VARLEN_AVAILABLE: return 1;
    default: return -1;
  }
}

int ffpa_attn_fwd_tile_config(int head_dim, int* block_rows, int* block_keys, int* lds_bytes) {
  const DimEntry* de = find_dim(head_dim);
  if (de == nullptr) return fail(FFPA_ERR_BAD_HEADDIM, "headdim not support! D=%d", head_dim);
  int br = 0, bc = 0, lds = 0;
  de->config(0, &br, &bc, &lds);
  if (block_rows) *block_rows = br;
  if (block_keys) *block_keys = bc;
  if (lds_bytes) *lds_bytes = lds;
  return FFPA_OK;
}

const char* ffpa_attn_last_error(void) { return g_err; }

#ifdef FFPA_PRODUCT_BUILD
const char* ffpa_attn_version(void) { return "ffpa-attn-amd 0.5.0 gfx950"; }
#else
const char* ffpa_attn_version(void) { return "ffpa-attn-amd 0.5.0 gfx950 (developer variant: NOT a product build)"; }
#endif

}  // extern "C"
