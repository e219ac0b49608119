// Batched weighted edit distance (Wagner-Fischer with ins=1, del=1, sub=2, and
// as a second metric unit-cost Levenshtein distance) and fused closest-match
// search on MI355X (gfx950).
//
// Used by the fuzzy matcher behind common.GetClosestMatchingString
// (reference internal/common/utils.go:377-401), which the CF container-types
// collector (internal/collector/cfcontainertypescollector.go:110-124) runs for
// every (buildpack name x builder buildpack) pair.  On a CF foundation export
// this is a |names| x |buildpacks| all-pairs problem.
//
// With substitution cost == insertion + deletion the weighted distance is
// exactly  |a| + |b| - 2 * LCS(a, b),  so each pair reduces to Hyyro's
// bit-parallel LCS over a DP column of |query| bits: one machine word for
// queries <= 64 bytes, 2 or 4 u64 words with a carry chain up to 256 bytes.
//
// Layout (CDNA4-first; every step below was kept or dropped on rocprofv3
// numbers, see profiles/r01_ed_kernel*):
//  * Byte remap.  The host assigns every byte value that occurs a dense code,
//    most frequent option byte first, code 0 = padding, and (<= 63 symbols)
//    stores code*4 so the LDS byte address of a character is one VALU op.
//    Masks of code 0 are 0, so padding leaves a column unchanged: no
//    per-character length checks.
//  * Query tiles.  Queries are sorted by length and grouped so one pass over
//    the option characters serves several queries: 8 queries <= 16 bytes
//    (two per 32-bit word, v_pk_add_u16 keeps the halves independent),
//    4 <= 32 bytes (one per word) or 2 <= 64 bytes (one u64 each).
//  * One table scheme for every class (TileDesc).  The query in slot s of a
//    tile owns column bits [s*MAXLEN, (s+1)*MAXLEN) of the tile's column.  The
//    masks are staged in LDS as NSUB = NQ*MAXLEN/64 sub-tables of 256 u64
//    entries (2 KiB each): entry c of sub-table h = bits [64h, 64h+64) of
//    code c's match mask, so a character costs NSUB conflict-free ds_read_b64
//    (banked mod 64 over 32-lane groups): two (4 KiB) for the classes up to
//    64 bytes, four (8 KiB) for the wide ones.  In the staging/device buffer
//    the tables lie in class order, each class a run of equally sized tables;
//    a launch gets pointers to its first tile's tables and tileQ/tileLen rows
//    and blockIdx.y counts tiles from there.
//  * Wide tiles (queries of 65..256 bytes).  K128 = 2 queries of <= 128 bytes
//    (2 u64 column words each), K256 = 1 query of <= 256 bytes (4 words).
//    Same data movement for both: four ds_read_b64 and four word steps per
//    character.  Only the addition links a query's words: one v_add_co_u32 +
//    3 (K128) or 7 (K256) v_addc_co_u32 per query and character; the carry out
//    of the top word is dropped and the classes differ in nothing else.
//    ISA as compiled (hipcc -O3, gfx950, read from -save-temps), per 32
//    characters (two options x 16) of the closest kernels: 128 ds_read_b64 and
//    no ds_read2st64_b64, 256 v_bitop3_b32, 64 v_add_co + 192 v_addc_co (K128)
//    or 32 + 224 (K256), no compare-and-select carries, no scratch.  VGPRs:
//    closest K128 56, K256 58; matrix K128 53, K256 57 (K64: 43 / 41), 8
//    waves/SIMD for all.  The 64-bit __builtin_addcll did not give this (see
//    lcs_step_wide).  Measured (200k options x 2048 queries, MI355X): 0.203
//    (K128) and 0.200 ps (K256) of closest-kernel time per option byte x query
//    x u64 column word against K64's 0.231, see docs/history.md.
//  * LCS step.  U = V & M; V' = (V + U) | (V & ~M)  (V - U never borrows
//    because U is a subset of V) = and + add + one v_bitop3_b32 per word.
//  * Options are sorted by length and cut into panels of 512 (256 threads x 2
//    options each: two independent chains per lane).  A panel is stored as
//    16-byte blocks [block][slot]: one global_load_dwordx4 gives a lane its
//    next 16 characters, and the next block is prefetched while the current
//    one is consumed.  blockIdx.x walks panels, remapped XCD-aware
//    (consecutive panels of one tile on one XCD's L2).
//  * ed_closest fuses the argmin: key = (dist << 32 | original index), min
//    over the wave by shuffles, over the 4 waves in LDS, then one 64-bit
//    atomicMin per query per workgroup, so only (index, dist) pairs leave
//    the GPU.  Ties resolve to the lowest index, like the reference's scan.
//  * ed_matrix writes a query-major [nB][nA] matrix (Python returns the
//    transposed view); it is bound by the scattered int32 stores and, end to
//    end, by the device-to-host copy of the matrix itself.
//  * Tiles are launched in slabs of <= 65535 (gridDim.y limit).
//
// Second metric: unit-cost Levenshtein distance (ins = del = sub = 1), the
// METRIC template parameter of both kernels and of for_each_option.  It is
// Myers' bit-vector recurrence in Hyyro's form with the DP column over the
// query: two vectors per column word, Pv (vertical +1) and Mv (vertical -1),
// from Pv = ~0, Mv = 0, and after the option's last character
//   dist = |a| + popc(Pv & mask(len)) - popc(Mv & mask(len)).
// Code map, panels (host or device fill), mask tables in LDS, the ds_read_b64
// scheme, the XCD remap, the argmin and the slab launches are the LCS
// kernels'; the host side does not know the metric until it launches.  What
// is this family's own:
//  * Padding is not neutral.  A character that matches nothing still adds a DP
//    column, so a lane steps exactly lenSorted[slot] characters (read before
//    the panel walk).  Chosen shape, at 4-character granularity because a
//    lane's 16-byte block arrives as four words: a word that both of the
//    lane's options still fill goes through the unrolled path with the two
//    chains interleaved; the one word in which an option ends runs a counted
//    loop of <= 3 steps under the exec mask; words behind the end do nothing,
//    and a lane stops loading blocks after its longer option's last one.
//    Per-character predication of the state was not built: it costs two
//    v_cndmask_b32 per column word and character (a fifth on top of the ten
//    below) on every character, and steps through all padding besides.
//  * Word steps (myers_step16 / myers_step).  K16 keeps two queries per word
//    with v_pk_add_u16 and v_pk_lshlrev_b16 and ors 0x00010001 into Ph.  Every
//    other class is a run of 32-bit words per query (1, 2, 4, 8): the add is
//    v_add_co_u32 + v_addc_co_u32 (__builtin_addc, as in lcs_step_wide), both
//    shifts take the bit from the word below with one v_alignbit_b32, and the
//    three-input forms are v_bitop3_b32.
//  * Registers.  Four state vectors per lane (Pv, Mv x two options) instead of
//    two.  Every class keeps two options per lane and compiles without
//    scratch, K256 included (96 VGPRs), so no class was cut to one option.
//    As compiled (hipcc -O3, gfx950, -save-temps), matrix / closest kernels,
//    the same for SCALED and not:
//             VGPR      SGPR      LDS bytes     scratch
//      K16    64 / 80   74 / 50   4096 / 4352   0
//      K32    64 / 72   54 / 42   4096 / 4224   0
//      K64    64 / 68   46 / 42   4096 / 4160   0
//      K128   93 / 97   50 / 46   8192 / 8256   0
//      K256   94 / 96   46 / 47   8192 / 8224   0
//    (Fewer resident waves than the LCS kernels' 8 per SIMD wherever a
//    kernel takes more than 64 VGPRs.)  The 20 LCS kernels keep their
//    figures: VGPR 39/39/41/53/57 matrix and 54/46/43/56/58 closest, no
//    scratch.
//  * Instruction mix, closest kernels, over the kernel's 40 character bodies
//    (32 unrolled + 8 in the counted loops).  K32 (4 column words): 80
//    ds_read_b64, 640 v_bitop3_b32, 355 v_and_b32, 363 v_or_b32, 344
//    v_lshlrev_b32, 179 v_add_u32: 11.6 VALU per word and character (the
//    compiler folds Mv' = Ph & (Eq | Mv) into a fourth bitop3 and splits
//    (Ph << 1) | 1 into shift + or).  K256 (8 words, one query): 160
//    ds_read_b64, 1280 v_bitop3_b32, 690 v_and_b32, 482 v_or_b32, 560
//    v_alignbit_b32, 43 v_add_co_u32 + 282 v_addc_co_u32, 103 v_lshlrev_b32:
//    10.8 per word and character; no compare-and-select carries.
//  * Measured (200k options x 2048 queries, MI355X, closest kernels, ps per
//    option byte x query x u64 column word): K16 0.67, K32 0.62, K64 0.58,
//    K128 0.56, K256 0.53 against the LCS kernels' 0.32 / 0.23 / 0.24 / 0.22 /
//    0.21 in the same runs: 2.1 to 2.7 times the LCS time per character.  See
//    docs/history.md.
//
// Third family: the closest option of every group (ed_closest_grouped_kernel,
// both metrics, every class and scaling: 20 kernels).  The matcher's caller has
// G groups of options (the buildpacks of G builders) and wants the closest one
// of each group; with the closest kernels that is G requests, each with its own
// query preparation, copies and launches.  Here the options carry a group id
// and one pass answers best[q * nGroups + g], the closest kernels' key.
//  * Order and panels.  The options are sorted by (group, length), stable, and
//    packed back to back into the same panels of 512: small groups share a
//    panel, a large group's panels are uniform in group and sorted by length
//    like today's.  panelBlocks[p] is the maximum over the panel's slots (the
//    last slot need not be the longest).  One more array is copied,
//    groupSorted[slot], -1 for an empty slot.  Code map, tables, host and
//    device fill do not know about groups.
//  * Reduction.  A lane folds its two options into key[NQ] as in ed_closest;
//    the wave keeps one held group for those keys, in an SGPR (readlane /
//    readfirstlane), so every branch on it is scalar.  Per panel and option the
//    wave ballots its 64 slots' groups:
//      all live slots in the held group  fold (the only path of a large group:
//                                        one load, two compares, one s_and)
//      all in one other group            flush, hold that group, fold
//      mixed (a boundary in the wave)    every live lane sends its own
//                                        atomicMin per query; the held stays
//    A flush is the shuffle min over the wave, one 64-bit atomicMin per query
//    from lane 0, keys back to ~0; the wave flushes once more after its last
//    panel.  No LDS stage across the four waves: they may hold different
//    groups (4 x NQ atomics per workgroup at the end instead of NQ).
//  * Traps.  The shuffles need all 64 lanes active, so the flush sits in
//    wave-uniform control flow: the kernel walks the panels itself (over the
//    shared panel_lcs / panel_lev / query_lcs / query_lev) and takes its
//    decisions outside the per-lane `live` test; for_each_option calls back
//    behind `if (o < 0) continue`.  Empty slots (group -1) never fold and never
//    count as another group.  Ties go to the lowest original index through the
//    key, whatever order the atomics land in.
//  * As compiled (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage),
//    LCS / Levenshtein kernels, the same for SCALED and not, no scratch:
//             VGPR      SGPR       LDS bytes
//      K16    58 / 82   106 / 105  4096
//      K32    50 / 74   70 / 72    4096
//      K64    48 / 70   54 / 58    4096
//      K128   60 / 99   58 / 62    8192
//      K256   62 / 98   50 / 55    8192
//    (2 to 5 VGPRs over the closest kernels, which costs one resident wave per
//    SIMD where it crosses a step of 8: LCS K16 7 waves; Levenshtein K16 5,
//    K32 6, K256 4; the other six keep the closest kernels' count.)  The branches on the ballots and on the held group
//    compile to s_cbranch_scc / vcc, the held group lives in an SGPR.  The 40
//    other matcher kernels and ed_fill_panels_kernel keep their figures.
//  * Measured (200k options x 2048 queries, raw names, MI355X, see
//    docs/history.md): with one group the kernels take 1.006 times the closest
//    kernels' time; 8 groups in one call 1.8 times, 64 groups 6 to 7 times
//    faster end to end than one closest call per group.
//
// Fourth family: the k closest options of every query, k <= K_MAX = 64
// (ed_topk_kernel, both metrics, every class and scaling: 20 kernels, and one
// ed_topk_merge_kernel).  A ranked list through ed_matrix is nA x nB stores, the
// copy of the matrix and a host selection per column; the closest kernels'
// 64-bit atomicMin keeps one key.  Here the selection runs in registers next to
// the distance work and only k keys per query leave the GPU, in (distance,
// index) order: the closest kernels' key, so rank 0 is ed_closest's answer.
//  * Work split, panels, tables, column steps, XCD remap and slabs are the
//    other families'.  The kernel walks the panels itself like the grouped one:
//    the selection uses cross-lane operations and sits in wave-uniform control
//    flow, not behind for_each_option's per-lane skip.
//  * The list.  Each wave keeps, for every query of the tile, its best 64 keys
//    as one u64 per lane: lane r holds rank r, ascending, ~0 = no entry (2 VGPRs
//    per query, 16 for K16).  tau[j] = the key at rank k-1 (v_readlane_b32 x 2),
//    wave-uniform in SGPRs, ~0 at the start; 0 for an empty query slot, which
//    then admits nothing.
//  * Filter.  Per panel and option a lane forms its NQ keys (~0 for an empty
//    slot), compares each as a full 64-bit key with tau[j] (v_cmp_lt_u64 against
//    an SGPR pair) and ors the predicates; one ballot per option decides, and
//    when it is zero - the steady state - nothing else runs.
//  * Insert (topk_offer / topk_insert).  Otherwise, per query, a scalar loop
//    over the set bits of that query's ballot: broadcast the lane's key x
//    (readlane), prev = the list shifted up one lane (v_mov_b32_dpp wave_shr:1,
//    lane 0 sees 0), l' = l < x ? l : (prev < x ? x : prev), refresh tau[j], and
//    ballot the remaining candidates against the new tau, so every pass of the
//    loop inserts.  Keys are distinct (the index is part of them): the order is
//    total and independent of arrival.  No LDS beyond the mask tables, no
//    ds_bpermute, no atomics.
//  * Write-out.  After its last panel a wave stores ranks 0 .. k-1 of every
//    query, lane r rank r (coalesced), to part[slot][p][rank]: slot = the query's
//    place in its class (tile * NQ + j), p over the class's gridDim.x * 4 waves.
//    The partial buffer is device-only (Arena::out, which a matrix request uses
//    for its output), planned on the host per class (Layout::partOff /
//    partCount, from grid_x) and cleared to 0xff on the stream before the
//    launches.  The four waves of a workgroup are not merged in LDS first.
//  * Merge.  One launch per class, one wave per query slot: it reads the
//    slot's parts 64 keys at a time (coalesced), filters against its tau and
//    inserts with the same routine, then writes k keys to best[query][rank],
//    which the host unpacks like the closest kernels' `best` (~0 = -1 / -1).
//  * As compiled (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage),
//    LCS / Levenshtein kernels, the same for SCALED and not, no scratch:
//             VGPR      SGPR      LDS bytes   waves/SIMD
//      K16    72 / 96   64 / 58   4096        7 / 5
//      K32    56 / 80   48 / 44   4096        8 / 6
//      K64    49 / 72   42 / 44   4096        8 / 7
//      K128   60 / 99   48 / 50   8192        8 / 4
//      K256   60 / 96   46 / 50   8192        8 / 5
//    ed_topk_merge_kernel: 14 VGPRs, 22 SGPRs, no LDS, no scratch.  The loops of
//    topk_offer branch on s_cmp_lg_u64 / vcc of SGPR values only.  The 61 other
//    kernels keep their VGPR, SGPR, LDS and scratch figures.
//  * Measured (200k options x 2048 raw names, MI355X, see docs/history.md):
//    k = 1 takes 1.03 times the closest kernels' time, k = 8 1.13, k = 64 1.64
//    (the first panel fills the list by k serial inserts per query and wave,
//    and K16 has eight queries); against ed_matrix plus a host selection the
//    call is 58 to 66 times faster end to end.
//
// Fifth family: many names against a few options (ed_closest_names_kernel,
// both metrics, every class and scaling: 20 kernels; an ungrouped request is a
// grouped one with one group).  The four families above put the options in the
// lanes and the queries' tables in LDS; with a few dozen options that is one
// panel with most lanes empty, and a table staged per 8 queries.  Both metrics
// have ins = del, so dist(a, b) = dist(b, a) and the roles can be swapped: here
// the names are the panel side (sorted by length, 512 to a panel, two per lane,
// host or device fill as before) and the options the tile side.  The 256-byte
// limit moves to the options with the column; a name can be of any length.
// Reused as they are: panel_lcs / panel_lev / query_lcs / query_lev, the code
// map (ranked by the names' bytes, the side the lanes look up), the tables and
// the [block][slot] panels.  This family's own:
//  * Tile plan (plan_tiles_grouped).  Options ordered by (class, group, length),
//    stable; a tile is closed on a change of class or group and its remaining
//    slots stay empty, so a tile never holds two groups.  One more array,
//    tileGroup[t], is copied with tileQ / tileLen.
//  * Work split.  The grid is over panels only: one launch per class that has
//    tiles, no blockIdx.y.  A workgroup takes a panel (up to 4096 panels one
//    each, beyond that persistent and strided, XCD remap as above) and loops
//    over the class's tiles inside the kernel, so a lane's running minimum per
//    name never leaves its registers.  The tile index, tileGroup, tileQ /
//    tileLen and the held group come from kernel arguments and uniform loads:
//    SGPRs, scalar branches.
//  * LDS.  kNamesChunkBytes = 32 KiB of tables are resident at once, static: 8
//    tiles of the classes up to 64 bytes (64 / 32 / 16 options), 4 of the wide
//    ones (8 / 4 options).  A class that fits one chunk - a few dozen options,
//    the expected case - is staged once per workgroup before the panel loop,
//    otherwise per (panel, chunk) between two barriers (8 uint4 loads per lane
//    against 2 names x ~25 characters x 8 tiles x NSUB ds_read_b64: a few per
//    cent).  gfx950 has 160 KiB of LDS per CU (the compiler's occupancy figure
//    below is 160 / 32 = 5), so 32 KiB leaves 5 resident workgroups of 4 waves
//    = 5 waves per SIMD: what the Levenshtein kernels' VGPRs allow anyway (4 to
//    5), and 3 below the 8 the LCS kernels' 62 to 80 VGPRs would.  16 KiB would
//    keep all 8 but puts the collector's grouped shape (8 groups: 8 tiles per
//    class) on the per-panel path; above 64 KiB needs dynamic LDS and larger
//    workgroups for 2 resident ones.  Not measured against each other.  The
//    ds_read_b64 scheme and the empty-asm barrier are step4's / lev_char's; a
//    tile's base is one more scalar term of the address.
//  * Names are read again for every tile (the panel is L1 / L2 resident after
//    the first).  Holding short names' blocks in registers across tiles was not
//    built.
//  * Reduction.  None across lanes: no shuffles, no LDS stage, no ballots.  A
//    lane folds a tile's NQ distances into key = (dist << 32 | original option
//    index) of the held group (ties to the lowest index whatever the tile
//    order), and when tileGroup changes, and after the last tile, commits it
//    to best[name * nGroups + group] (preset to ~0) by a plain load / min /
//    store: one lane of one workgroup owns the entry within a launch, and the
//    class launches of a request are ordered on its stream, so no atomic is
//    needed.  Empty tile slots and empty panel slots contribute nothing.
//  * As compiled (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage),
//    LCS / Levenshtein kernels, the same for SCALED and not, no scratch:
//             VGPR       SGPR      LDS bytes   waves/SIMD
//      K16    62 / 76    60 / 63   32768       5 / 5
//      K32    62 / 77    60 / 62   32768       5 / 5
//      K64    63 / 78    60 / 62   32768       5 / 5
//      K128   76 / 107   61 / 62   32768       5 / 4
//      K256   80 / 109   61 / 62   32768       5 / 4
//    The 82 other kernels keep their VGPR, SGPR, LDS and scratch figures.
//  * Measured (1M raw names, 4 to 64 bytes, MI355X, see docs/history.md): 64
//    options, kernel time 0.48 ms against the closest kernels' 3.1 to 3.2 ms
//    (8 groups: 0.82 against the grouped kernels' 3.6; Levenshtein 1.02 against
//    2.26 and 1.51 against 3.10); end to end 24 to 36 ms against 157 to 176 ms,
//    because the host no longer builds a table per 2 to 8 names.  At 1M names
//    the kernel times meet at 1024 options (ungrouped) and stay level to 4096.
//    Over the name count they meet near 1024 names per option; with few names
//    the grid is a handful of workgroups and the other families' kernels are
//    faster.  The raw lines are in profiles/ed_names/.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <mutex>
#include <numeric>
#include <thread>
#include <vector>

#define THREADS 256
#define OPT_PER_THREAD 2
#define SLOTS (THREADS * OPT_PER_THREAD)
#define MAX_Y 65535

typedef unsigned long long u64;

namespace {

__device__ __forceinline__ int remap_panel(int bx, int n) {
  if (n % 8 != 0) return bx;
  const int per = n / 8;
  return (bx % 8) * per + (bx / 8);
}

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// Tile kinds: how many queries share one pass over the option characters.
//   K16: 8 queries <= 16 bytes, two per 32-bit word (v_pk_add_u16/v_pk_sub_u16
//        keep the halves independent, exactly two 16-bit LCS columns)
//   K32: 4 queries <= 32 bytes, one per 32-bit word
//   K64: 2 queries <= 64 bytes, one per 64-bit word
//   K128: 2 queries of 65..128 bytes, two u64 words each  } wide tiles: the add
//   K256: 1 query of 129..256 bytes, four u64 words       } carries across words
// A class chooses W (the register word of the column), NQ (queries per tile)
// and MAXLEN (longest query in bytes); the query in slot s owns column bits
// [s*MAXLEN, (s+1)*MAXLEN).  Derived: WPQ = u64 words per query (the length of
// the carry chain), NSUB = 2 KiB LDS sub-tables (one ds_read_b64 each per
// character), NW = column words, TABLE_BYTES / TABLE_U4 = one tile's mask
// tables.  The host side takes the classes from here too.
constexpr int kTableEntries = 256;                            // entries per sub-table: one per byte code
constexpr int kSubTableBytes = kTableEntries * sizeof(u64);  // 2 KiB
constexpr int kTileSlots = 8;                                 // slots per tile in tileQ / tileLen
template <class W_, int NQ_, int MAXLEN_>
struct TileDesc {
  typedef W_ W;
  enum {
    NQ = NQ_,
    MAXLEN = MAXLEN_,
    WPQ = MAXLEN > 64 ? MAXLEN / 64 : 1,
    NSUB = NQ * MAXLEN / 64,
    NW = NQ * MAXLEN / (8 * sizeof(W)),
    TABLE_BYTES = NSUB * kSubTableBytes,
    TABLE_U4 = TABLE_BYTES / sizeof(uint4)
  };
  static_assert(NSUB == 2 || NSUB == 4, "step4 reads 2 or 4 sub-tables per character");
  static_assert(NQ <= kTileSlots, "a tile's queries fit its tileQ / tileLen row");
  static_assert(MAXLEN <= 64 || (MAXLEN == 64 * WPQ && sizeof(W) == sizeof(u64)), "a wide query fills its u64 words");
};
enum { K16 = 0, K32 = 1, K64 = 2, K128 = 3, K256 = 4, NKINDS = 5 };
template <int KIND> struct TileT;
template <> struct TileT<K16> : TileDesc<uint32_t, 8, 16> {};
template <> struct TileT<K32> : TileDesc<uint32_t, 4, 32> {};
template <> struct TileT<K64> : TileDesc<u64, 2, 64> {};
template <> struct TileT<K128> : TileDesc<u64, 2, 128> {};
template <> struct TileT<K256> : TileDesc<u64, 1, 256> {};
static_assert(TileT<K16>::MAXLEN < TileT<K32>::MAXLEN && TileT<K32>::MAXLEN < TileT<K64>::MAXLEN &&
                  TileT<K64>::MAXLEN < TileT<K128>::MAXLEN && TileT<K128>::MAXLEN < TileT<K256>::MAXLEN,
              "the host picks the first class whose MAXLEN holds the query");

// One LCS step of a column word against its match mask.  Hyyro's
// V' = (V + U) | (V - U) with U = V & M; U's bits are a subset of V's, so
// V - U borrows nowhere and equals V & ~M:  V' = (V + U) | (V & ~M) - an and,
// an add and one 3-input v_bitop3_b32 per 32-bit word (v2 spent ~4.4 ops).
// f(A, V, M) = A | (V & ~M) as one v_bitop3_b32 (truth table 0xF4, operand
// bits indexing it as A*4 + V*2 + M); spelled out because the compiler emits
// v_bfi + v_or for the 64-bit halves.
__device__ __forceinline__ uint32_t or_andn(uint32_t a, uint32_t v, uint32_t m) {
  return __builtin_amdgcn_bitop3_b32(a, v, m, 0xF4);
}

__device__ __forceinline__ u64 or_andn64(u64 a, u64 v, u64 m) {
  return ((u64)or_andn((uint32_t)(a >> 32), (uint32_t)(v >> 32), (uint32_t)(m >> 32)) << 32) |
         or_andn((uint32_t)a, (uint32_t)v, (uint32_t)m);
}

template <int KIND>
__device__ __forceinline__ void lcs_step(typename TileT<KIND>::W &V, typename TileT<KIND>::W m) {
  typedef typename TileT<KIND>::W W;
  const W U = V & m;
  if constexpr (KIND == K16) {
    const uint32_t A = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, V) + __builtin_bit_cast(u16x2, U));
    V = or_andn(A, V, m);
  } else if constexpr (KIND == K32) {
    V = or_andn(V + U, V, m);
  } else {
    V = or_andn64(V + U, V, m);
  }
}

// The same step on a query's column of WPQ u64 words (wide tiles).  Only the
// addition links the words: V + U is one WPQ*64-bit sum (a v_add_co_u32 and a
// run of v_addc_co_u32), the carry out of the top word is dropped, and the
// V & ~M half stays word-local.  A padding character (every mask 0) has U = 0:
// no carry, V' = V | V.  Bits above the query's length never match, so a
// carry that ripples through them is put back by the | V term: they stay set
// and query_lcs masks them off.
// The sum is written over 32-bit halves with __builtin_addc: that is what the
// hardware's carry chain is made of, and the 64-bit __builtin_addcll came out
// as v_lshl_add_u64 + v_cmp_lt_u64 + v_cndmask carry emulation instead.
template <int WPQ>
__device__ __forceinline__ void lcs_step_wide(u64 *V, const u64 *m) {
  uint32_t A[2 * WPQ];
  unsigned carry = 0;
#pragma unroll
  for (int h = 0; h < 2 * WPQ; h++) {
    const uint32_t v = (uint32_t)(V[h / 2] >> (32 * (h & 1)));
    const uint32_t u = v & (uint32_t)(m[h / 2] >> (32 * (h & 1)));
    A[h] = __builtin_addc(v, u, carry, &carry);
  }
#pragma unroll
  for (int w = 0; w < WPQ; w++) V[w] = or_andn64(((u64)A[2 * w + 1] << 32) | A[2 * w], V[w], m[w]);
}

// Four coded characters of one option against every word of the tile.
//
// LDS layout (TABLE_BYTES per tile): NSUB sub-tables of kTableEntries u64
// entries, sub-table h at byte kSubTableBytes*h, entry c of sub-table h = bits
// [64h, 64h+64) of code c's mask over the tile's column.  In register words:
// K16/K32: words 2h (low half) and 2h+1 (high half); K64 and the wide tiles:
// column word h (K64: query h; K128: query h/2, word h%2; K256: word h of the
// one query).
// Each character costs NSUB `ds_read_b64` (bank = (addr/4) mod 64 over 32-lane
// groups, so the <= 32 most frequent codes never conflict; 2 LDS cycles each).
// Every address after the first goes through an empty asm so the compiler
// cannot fuse a pair into `ds_read2st64_b64` - that form banks mod 32 in
// 16-lane groups and cost 8 cycles + ~7 conflict cycles per instruction in
// PMC (v5).
template <int KIND, bool SCALED>
__device__ __forceinline__ void step4(uint32_t w, const char *T, typename TileT<KIND>::W (&V)[TileT<KIND>::NW]) {
  typedef TileT<KIND> TT;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint32_t c = (w >> (8 * i)) & 0xffu;
    const uint32_t off = SCALED ? c * 2u : c * 8u;  // byte offset of entry c in a u64 table
    uint32_t offh[TT::NSUB];
    u64 m[TT::NSUB];
    offh[0] = off;
#pragma unroll
    for (int h = 1; h < TT::NSUB; h++) {
      offh[h] = off + kSubTableBytes * h;
      __asm__ volatile("" : "+v"(offh[h]));
    }
#pragma unroll
    for (int h = 0; h < TT::NSUB; h++) m[h] = *reinterpret_cast<const u64 *>(T + offh[h]);
    if constexpr (TT::WPQ > 1) {
#pragma unroll
      for (int q = 0; q < TT::NQ; q++) lcs_step_wide<TT::WPQ>(&V[q * TT::WPQ], &m[q * TT::WPQ]);
    } else if constexpr (KIND == K64) {
      lcs_step<KIND>(V[0], m[0]);
      lcs_step<KIND>(V[1], m[1]);
    } else {
      lcs_step<KIND>(V[0], (uint32_t)m[0]);
      lcs_step<KIND>(V[1], (uint32_t)(m[0] >> 32));
      lcs_step<KIND>(V[2], (uint32_t)m[1]);
      lcs_step<KIND>(V[3], (uint32_t)(m[1] >> 32));
    }
  }
}

// LCS columns of this lane's OPT_PER_THREAD options in one panel against the tile.
template <int KIND, bool SCALED>
__device__ __forceinline__ void panel_lcs(const uint4 *__restrict__ panel, int blocks, const char *T,
                                          typename TileT<KIND>::W (&V)[OPT_PER_THREAD][TileT<KIND>::NW]) {
  typedef typename TileT<KIND>::W W;
  const int lane = threadIdx.x;
#pragma unroll
  for (int u = 0; u < OPT_PER_THREAD; u++)
#pragma unroll
    for (int k = 0; k < TileT<KIND>::NW; k++) V[u][k] = ~(W)0;
  if (blocks == 0) return;
  uint4 cur[OPT_PER_THREAD], nxt[OPT_PER_THREAD];
#pragma unroll
  for (int u = 0; u < OPT_PER_THREAD; u++) cur[u] = panel[u * THREADS + lane];
  for (int b = 0; b < blocks; b++) {
    if (b + 1 < blocks) {
#pragma unroll
      for (int u = 0; u < OPT_PER_THREAD; u++) nxt[u] = panel[(size_t)(b + 1) * SLOTS + u * THREADS + lane];
    }
    // the two options' chains interleave word by word
    step4<KIND, SCALED>(cur[0].x, T, V[0]);
    step4<KIND, SCALED>(cur[1].x, T, V[1]);
    step4<KIND, SCALED>(cur[0].y, T, V[0]);
    step4<KIND, SCALED>(cur[1].y, T, V[1]);
    step4<KIND, SCALED>(cur[0].z, T, V[0]);
    step4<KIND, SCALED>(cur[1].z, T, V[1]);
    step4<KIND, SCALED>(cur[0].w, T, V[0]);
    step4<KIND, SCALED>(cur[1].w, T, V[1]);
#pragma unroll
    for (int u = 0; u < OPT_PER_THREAD; u++) cur[u] = nxt[u];
  }
}

// LCS length of tile query j from the final column words.
template <int KIND>
__device__ __forceinline__ int query_lcs(const typename TileT<KIND>::W (&V)[TileT<KIND>::NW], int j, int len) {
  if constexpr (KIND == K16) {
    const uint32_t bits = (~V[j >> 1] >> (16 * (j & 1))) & ((1u << len) - 1u);  // len <= 16
    return __popc(bits);
  } else if constexpr (KIND == K32) {
    const uint32_t mask = len >= 32 ? ~0u : ((1u << len) - 1u);
    return __popc(~V[j] & mask);
  } else if constexpr (KIND == K64) {
    const u64 mask = len >= 64 ? ~0ULL : ((1ULL << len) - 1ULL);
    return __popcll(~V[j] & mask);
  } else {
    // wide: popcounts over the query's words, the length mask on the last one
    // (an empty slot has len 0: every word is masked to nothing)
    int n = 0;
#pragma unroll
    for (int w = 0; w < TileT<KIND>::WPQ; w++) {
      const int bits = len - 64 * w;
      const u64 mask = bits >= 64 ? ~0ULL : (bits <= 0 ? 0ULL : ((1ULL << bits) - 1ULL));
      n += __popcll(~V[j * TileT<KIND>::WPQ + w] & mask);
    }
    return n;
  }
}

// ---------------------------------------------------------------------------
// The second metric: unit-cost Levenshtein distance (ins = del = sub = 1) by
// Myers' bit-vector recurrence in Hyyro's form.  Tables, panels and tiles are
// the LCS kernels'; what differs is the column (two vectors: Pv = vertical +1,
// Mv = vertical -1), the step, and that a lane counts its characters.
// ---------------------------------------------------------------------------
enum { METRIC_INDEL2 = 0, METRIC_LEVENSHTEIN = 1 };

// v_bitop3_b32 truth tables, written over the operands' own tables.
enum { BIT_A = 0xF0, BIT_B = 0xCC, BIT_C = 0xAA };
constexpr int kXorOr = ((BIT_A ^ BIT_B) | BIT_C) & 0xFF;   // (a ^ b) | c
constexpr int kOrNor = (BIT_A | ~(BIT_B | BIT_C)) & 0xFF;  // a | ~(b | c)

// The column of one option against a tile, in 32-bit words: NH = 2 per
// sub-table, HPQ of them to a query (K16: two queries to a word instead).
template <int KIND>
struct LevColumn {
  enum { NH = 2 * TileT<KIND>::NSUB, HPQ = KIND == K16 ? 1 : TileT<KIND>::MAXLEN / 32 };
  uint32_t Pv[NH], Mv[NH];
};

// One character against the two 16-bit columns of a K16 word: the add and both
// shifts are packed 16-bit operations, so nothing crosses from the low query
// into the high one, and each half of Ph gets its own 1.
__device__ __forceinline__ void myers_step16(uint32_t &Pv, uint32_t &Mv, uint32_t eq) {
  const uint32_t sum = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, eq & Pv) + __builtin_bit_cast(u16x2, Pv));
  const uint32_t xh = __builtin_amdgcn_bitop3_b32(sum, Pv, eq, kXorOr);
  const uint32_t ph = __builtin_amdgcn_bitop3_b32(Mv, xh, Pv, kOrNor);
  const uint32_t mh = Pv & xh;
  const uint32_t phs = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, ph) << 1) | 0x00010001u;
  const uint32_t mhs = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, mh) << 1);
  const uint32_t xv = eq | Mv;
  Pv = __builtin_amdgcn_bitop3_b32(mhs, xv, phs, kOrNor);
  Mv = phs & xv;
}

// One character against a query's column of N 32-bit words (N = 1 for K32 up
// to 8 for K256).  Two things link the words, both upward only: the addition
// (v_add_co_u32 + v_addc_co_u32, the carry out of the top word is dropped) and
// the two shifts, which take bit 31 of the word below through v_alignbit_b32;
// the lowest word of Ph shifts a 1 in (v_lshl_or_b32).  Ten VALU operations
// per word whatever N is.  Bits above the query's length hold garbage that
// never comes down; query_lev masks it off.
template <int N>
__device__ __forceinline__ void myers_step(uint32_t *Pv, uint32_t *Mv, const uint32_t *eq) {
  uint32_t xh[N];
  unsigned carry = 0;
#pragma unroll
  for (int h = 0; h < N; h++) {
    const uint32_t sum = __builtin_addc(eq[h] & Pv[h], Pv[h], carry, &carry);
    xh[h] = __builtin_amdgcn_bitop3_b32(sum, Pv[h], eq[h], kXorOr);
  }
  uint32_t phBelow = 0, mhBelow = 0;
#pragma unroll
  for (int h = 0; h < N; h++) {
    const uint32_t ph = __builtin_amdgcn_bitop3_b32(Mv[h], xh[h], Pv[h], kOrNor);
    const uint32_t mh = Pv[h] & xh[h];
    const uint32_t phs = h == 0 ? (ph << 1) | 1u : __builtin_amdgcn_alignbit(ph, phBelow, 31);
    const uint32_t mhs = h == 0 ? mh << 1 : __builtin_amdgcn_alignbit(mh, mhBelow, 31);
    phBelow = ph;
    mhBelow = mh;
    const uint32_t xv = eq[h] | Mv[h];
    Pv[h] = __builtin_amdgcn_bitop3_b32(mhs, xv, phs, kOrNor);
    Mv[h] = phs & xv;
  }
}

// One coded character against every query of the tile: the LDS reads of step4
// (same offsets, same conflict-free ds_read_b64), then the Myers steps.
template <int KIND, bool SCALED>
__device__ __forceinline__ void lev_char(uint32_t c, const char *T, LevColumn<KIND> &C) {
  typedef TileT<KIND> TT;
  typedef LevColumn<KIND> Col;
  const uint32_t off = SCALED ? c * 2u : c * 8u;
  uint32_t offh[TT::NSUB], eq[Col::NH];
  offh[0] = off;
#pragma unroll
  for (int h = 1; h < TT::NSUB; h++) {
    offh[h] = off + kSubTableBytes * h;
    __asm__ volatile("" : "+v"(offh[h]));
  }
#pragma unroll
  for (int h = 0; h < TT::NSUB; h++) {
    const u64 m = *reinterpret_cast<const u64 *>(T + offh[h]);
    eq[2 * h] = (uint32_t)m;
    eq[2 * h + 1] = (uint32_t)(m >> 32);
  }
  if constexpr (KIND == K16) {
#pragma unroll
    for (int k = 0; k < Col::NH; k++) myers_step16(C.Pv[k], C.Mv[k], eq[k]);
  } else {
#pragma unroll
    for (int q = 0; q < Col::NH; q += Col::HPQ) myers_step<Col::HPQ>(&C.Pv[q], &C.Mv[q], &eq[q]);
  }
}

// Four characters of both of the lane's options (word `w0` of option 0's
// block, `w1` of option 1's), of which the options still have r0 and r1 left
// (<= 0: the option ended).  A padding character is not neutral here - it
// would add a DP column - so a lane steps exactly its option's length: whole
// words go through the unrolled path, the two chains interleaved as in
// panel_lcs; the one word in which an option ends runs a counted loop of at
// most three steps under the exec mask, and words behind the end do nothing.
// Options of a panel are sorted by length, so a wave's lanes nearly always
// take the same side.
template <int KIND, bool SCALED>
__device__ __forceinline__ void lev_word(uint32_t w0, uint32_t w1, int r0, int r1, const char *T,
                                         LevColumn<KIND> (&C)[OPT_PER_THREAD]) {
  if (r0 >= 4 && r1 >= 4) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      lev_char<KIND, SCALED>((w0 >> (8 * i)) & 0xffu, T, C[0]);
      lev_char<KIND, SCALED>((w1 >> (8 * i)) & 0xffu, T, C[1]);
    }
  } else {
    const uint32_t w[OPT_PER_THREAD] = {w0, w1};
    const int r[OPT_PER_THREAD] = {r0, r1};
#pragma unroll
    for (int u = 0; u < OPT_PER_THREAD; u++) {
      uint32_t rest = w[u];
      const int n = r[u] < 4 ? r[u] : 4;
#pragma clang loop unroll(disable)
      for (int i = 0; i < n; i++) {
        lev_char<KIND, SCALED>(rest & 0xffu, T, C[u]);
        rest >>= 8;
      }
    }
  }
}

// Myers columns of this lane's OPT_PER_THREAD options (lengths la[u], in hand
// before the walk) in one panel against the tile.  The lane walks the blocks
// its longer option needs, never more than the panel has.
template <int KIND, bool SCALED>
__device__ __forceinline__ void panel_lev(const uint4 *__restrict__ panel, int blocks, const char *T,
                                          const int (&la)[OPT_PER_THREAD], LevColumn<KIND> (&C)[OPT_PER_THREAD]) {
  static_assert(OPT_PER_THREAD == 2, "lev_word takes the lane's two options");
  const int lane = threadIdx.x;
#pragma unroll
  for (int u = 0; u < OPT_PER_THREAD; u++)
#pragma unroll
    for (int k = 0; k < LevColumn<KIND>::NH; k++) {
      C[u].Pv[k] = ~0u;
      C[u].Mv[k] = 0u;
    }
  const int mine = ((la[0] > la[1] ? la[0] : la[1]) + 15) >> 4;
  const int n = mine < blocks ? mine : blocks;
  if (n == 0) return;
  uint4 cur[OPT_PER_THREAD], nxt[OPT_PER_THREAD];
#pragma unroll
  for (int u = 0; u < OPT_PER_THREAD; u++) cur[u] = panel[u * THREADS + lane];
  for (int b = 0; b < n; b++) {
    if (b + 1 < n) {
#pragma unroll
      for (int u = 0; u < OPT_PER_THREAD; u++) nxt[u] = panel[(size_t)(b + 1) * SLOTS + u * THREADS + lane];
    }
    const int r0 = la[0] - 16 * b, r1 = la[1] - 16 * b;
    lev_word<KIND, SCALED>(cur[0].x, cur[1].x, r0, r1, T, C);
    lev_word<KIND, SCALED>(cur[0].y, cur[1].y, r0 - 4, r1 - 4, T, C);
    lev_word<KIND, SCALED>(cur[0].z, cur[1].z, r0 - 8, r1 - 8, T, C);
    lev_word<KIND, SCALED>(cur[0].w, cur[1].w, r0 - 12, r1 - 12, T, C);
#pragma unroll
    for (int u = 0; u < OPT_PER_THREAD; u++) cur[u] = nxt[u];
  }
}

// Distance of tile query j (length len) to an option of length la from the
// final column: the bottom cell is la (the top row's value) plus the column's
// vertical deltas over the query's own bits.
template <int KIND>
__device__ __forceinline__ int query_lev(const LevColumn<KIND> &C, int j, int len, int la) {
  if constexpr (KIND == K16) {
    const uint32_t mask = (1u << len) - 1u;  // len <= 16
    const int sh = 16 * (j & 1);
    return la + __popc((C.Pv[j >> 1] >> sh) & mask) - __popc((C.Mv[j >> 1] >> sh) & mask);
  } else {
    int d = la;
#pragma unroll
    for (int h = 0; h < LevColumn<KIND>::HPQ; h++) {
      const int bits = len - 32 * h;
      const uint32_t mask = bits >= 32 ? ~0u : (bits <= 0 ? 0u : ((1u << bits) - 1u));
      d += __popc(C.Pv[j * LevColumn<KIND>::HPQ + h] & mask) - __popc(C.Mv[j * LevColumn<KIND>::HPQ + h] & mask);
    }
    return d;
  }
}

// Stage the tile's mask tables in LDS.  `tileM` is the table of the launch's
// first tile and the launch's tiles are one class, so tile number `tile` of
// the launch (blockIdx.y) lies `tile` tables further on.
template <int KIND>
__device__ __forceinline__ void load_tile(const uint4 *__restrict__ tileM, int tile, uint4 *T) {
  const uint4 *src = tileM + (size_t)tile * TileT<KIND>::TABLE_U4;
  for (int i = threadIdx.x; i < TileT<KIND>::TABLE_U4; i += THREADS) T[i] = src[i];
  __syncthreads();
}

// What both kernels do: stage the tile's tables, walk this workgroup's panels
// and, for every real option slot of the lane, call f(o, dist) with the
// option's original index and dist(j) = its distance to the tile's query j.
// Tile metadata: tileQ[t][kTileSlots] = query index (-1 = empty), tileLen[t][kTileSlots]
// = its length, t counted from the launch's first tile like the tables.
template <int KIND, bool SCALED, int METRIC, class F>
__device__ __forceinline__ void for_each_option(
    const uint4 *__restrict__ panels, const int64_t *__restrict__ panelOff, const int *__restrict__ panelBlocks,
    const int *__restrict__ lenSorted, const int *__restrict__ perm, const uint4 *__restrict__ tileM,
    const int *__restrict__ tileLen, int nPanels, F f) {
  typedef TileT<KIND> TT;
  __shared__ uint4 T[TT::TABLE_U4];
  const int tile = blockIdx.y;
  load_tile<KIND>(tileM, tile, T);
  int qlen[TT::NQ];
#pragma unroll
  for (int j = 0; j < TT::NQ; j++) qlen[j] = tileLen[tile * kTileSlots + j];
  for (int p = remap_panel(blockIdx.x, gridDim.x); p < nPanels; p += gridDim.x) {
    if constexpr (METRIC == METRIC_LEVENSHTEIN) {
      int la[OPT_PER_THREAD];  // an empty slot has length 0: it steps nothing
#pragma unroll
      for (int u = 0; u < OPT_PER_THREAD; u++) la[u] = lenSorted[p * SLOTS + u * THREADS + threadIdx.x];
      LevColumn<KIND> C[OPT_PER_THREAD];
      panel_lev<KIND, SCALED>(panels + panelOff[p], panelBlocks[p], reinterpret_cast<const char *>(T), la, C);
#pragma unroll
      for (int u = 0; u < OPT_PER_THREAD; u++) {
        const int o = perm[p * SLOTS + u * THREADS + threadIdx.x];
        if (o < 0) continue;
        auto dist = [&](int j) __attribute__((always_inline)) { return query_lev<KIND>(C[u], j, qlen[j], la[u]); };
        f(o, dist);
      }
    } else {
      typename TT::W V[OPT_PER_THREAD][TT::NW];
      panel_lcs<KIND, SCALED>(panels + panelOff[p], panelBlocks[p], reinterpret_cast<const char *>(T), V);
#pragma unroll
      for (int u = 0; u < OPT_PER_THREAD; u++) {
        const int s = p * SLOTS + u * THREADS + threadIdx.x;
        const int o = perm[s];
        if (o < 0) continue;
        const int la = lenSorted[s];
        auto dist = [&](int j) __attribute__((always_inline)) {
          return la + qlen[j] - 2 * query_lcs<KIND>(V[u], j, qlen[j]);
        };
        f(o, dist);
      }
    }
  }
}

}  // namespace

template <int KIND, bool SCALED, int METRIC>
__global__ __launch_bounds__(THREADS) void ed_matrix_kernel(
    const uint4 *__restrict__ panels, const int64_t *__restrict__ panelOff, const int *__restrict__ panelBlocks,
    const int *__restrict__ lenSorted, const int *__restrict__ perm, const uint4 *__restrict__ tileM,
    const int *__restrict__ tileQ, const int *__restrict__ tileLen, int nA, int nPanels, int *__restrict__ outT) {
  typedef TileT<KIND> TT;
  const int tile = blockIdx.y;
  int qid[TT::NQ];
#pragma unroll
  for (int j = 0; j < TT::NQ; j++) qid[j] = tileQ[tile * kTileSlots + j];
  auto store = [&](int o, auto dist) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < TT::NQ; j++)
      if (qid[j] >= 0) outT[(size_t)qid[j] * nA + o] = dist(j);
  };
  for_each_option<KIND, SCALED, METRIC>(panels, panelOff, panelBlocks, lenSorted, perm, tileM, tileLen, nPanels, store);
}

template <int KIND, bool SCALED, int METRIC>
__global__ __launch_bounds__(THREADS) void ed_closest_kernel(
    const uint4 *__restrict__ panels, const int64_t *__restrict__ panelOff, const int *__restrict__ panelBlocks,
    const int *__restrict__ lenSorted, const int *__restrict__ perm, const uint4 *__restrict__ tileM,
    const int *__restrict__ tileQ, const int *__restrict__ tileLen, int nPanels, u64 *__restrict__ best) {
  typedef TileT<KIND> TT;
  __shared__ u64 red[THREADS / 64][TT::NQ];
  u64 key[TT::NQ];
#pragma unroll
  for (int j = 0; j < TT::NQ; j++) key[j] = ~0ULL;
  auto keep_min = [&](int o, auto dist) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < TT::NQ; j++) {
      const u64 k = ((u64)(unsigned)dist(j) << 32) | (unsigned)o;
      key[j] = k < key[j] ? k : key[j];
    }
  };
  for_each_option<KIND, SCALED, METRIC>(panels, panelOff, panelBlocks, lenSorted, perm, tileM, tileLen, nPanels, keep_min);
  // argmin per query: wave shuffles, then the 4 waves through LDS, one atomic each
#pragma unroll
  for (int j = 0; j < TT::NQ; j++) {
    u64 k = key[j];
    for (int off = 32; off > 0; off >>= 1) {
      const u64 o = __shfl_xor(k, off, 64);
      k = o < k ? o : k;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x / 64][j] = k;
  }
  __syncthreads();
  if (threadIdx.x < TT::NQ) {
    const int j = threadIdx.x;
    const int q = tileQ[(int)blockIdx.y * kTileSlots + j];  // (not a qid[j] array: a dynamic index would spill it)
    u64 k = red[0][j];
    for (int w = 1; w < THREADS / 64; w++) k = red[w][j] < k ? red[w][j] : k;
    if (q >= 0 && k != ~0ULL) atomicMin(&best[q], k);
  }
}

// The closest option of every group (see "Third family" in the file header):
// best[q * nGroups + g] = min over the options of group g of the closest
// kernels' key.  The panel walk is this kernel's own, because the reduction
// needs a hook per (panel, option) that every lane of the wave reaches:
// for_each_option calls back behind a per-lane skip.
template <int KIND, bool SCALED, int METRIC>
__global__ __launch_bounds__(THREADS) void ed_closest_grouped_kernel(
    const uint4 *__restrict__ panels, const int64_t *__restrict__ panelOff, const int *__restrict__ panelBlocks,
    const int *__restrict__ lenSorted, const int *__restrict__ perm, const int *__restrict__ groupSorted,
    const uint4 *__restrict__ tileM, const int *__restrict__ tileQ, const int *__restrict__ tileLen, int nPanels,
    int nGroups, u64 *__restrict__ best) {
  typedef TileT<KIND> TT;
  __shared__ uint4 T[TT::TABLE_U4];
  const int tile = blockIdx.y;
  load_tile<KIND>(tileM, tile, T);
  int qlen[TT::NQ], qid[TT::NQ];
#pragma unroll
  for (int j = 0; j < TT::NQ; j++) {
    qlen[j] = tileLen[tile * kTileSlots + j];
    qid[j] = tileQ[tile * kTileSlots + j];
  }
  u64 key[TT::NQ];
#pragma unroll
  for (int j = 0; j < TT::NQ; j++) key[j] = ~0ULL;
  int held = -1;  // the group of what key[] holds, the same for the whole wave; -1 = nothing

  // Runs with all 64 lanes active: min over the wave, one atomic per query, keys back to ~0.
  auto flush = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < TT::NQ; j++) {
      u64 k = key[j];
      for (int off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_xor(k, off, 64);
        k = o < k ? o : k;
      }
      if ((threadIdx.x & 63) == 0 && qid[j] >= 0 && k != ~0ULL) atomicMin(&best[(size_t)qid[j] * nGroups + held], k);
      key[j] = ~0ULL;
    }
  };
  // Slot s of this lane (empty: group -1), dist(j) = its distance to query j.
  // Every branch but the innermost `g >= 0` is on a ballot or on `held`: scalar.
  auto reduce = [&](int s, auto dist) __attribute__((always_inline)) {
    const int g = groupSorted[s];
    const u64 live = __builtin_amdgcn_ballot_w64(g >= 0);
    if (live == 0) return;
    bool fold = (__builtin_amdgcn_ballot_w64(g != held) & live) == 0;  // every live slot in the held group
    if (!fold) {
      const int g0 = __builtin_amdgcn_readlane(g, __builtin_ctzll(live));
      if ((__builtin_amdgcn_ballot_w64(g != g0) & live) == 0) {  // one other group: it becomes the held one
        if (held >= 0) flush();
        held = __builtin_amdgcn_readfirstlane(g0);
        fold = true;
      }
    }
    if (g < 0) return;
    const unsigned o = (unsigned)perm[s];
#pragma unroll
    for (int j = 0; j < TT::NQ; j++) {
      const u64 k = ((u64)(unsigned)dist(j) << 32) | o;
      if (fold)
        key[j] = k < key[j] ? k : key[j];
      else if (qid[j] >= 0)  // a group boundary inside these 64 slots: every lane for itself
        atomicMin(&best[(size_t)qid[j] * nGroups + g], k);
    }
  };

  for (int p = remap_panel(blockIdx.x, gridDim.x); p < nPanels; p += gridDim.x) {
    const int s0 = p * SLOTS + threadIdx.x;
    if constexpr (METRIC == METRIC_LEVENSHTEIN) {
      int la[OPT_PER_THREAD];
#pragma unroll
      for (int u = 0; u < OPT_PER_THREAD; u++) la[u] = lenSorted[s0 + u * THREADS];
      LevColumn<KIND> C[OPT_PER_THREAD];
      panel_lev<KIND, SCALED>(panels + panelOff[p], panelBlocks[p], reinterpret_cast<const char *>(T), la, C);
#pragma unroll
      for (int u = 0; u < OPT_PER_THREAD; u++)
        reduce(s0 + u * THREADS,
               [&](int j) __attribute__((always_inline)) { return query_lev<KIND>(C[u], j, qlen[j], la[u]); });
    } else {
      typename TT::W V[OPT_PER_THREAD][TT::NW];
      panel_lcs<KIND, SCALED>(panels + panelOff[p], panelBlocks[p], reinterpret_cast<const char *>(T), V);
#pragma unroll
      for (int u = 0; u < OPT_PER_THREAD; u++) {
        const int la = lenSorted[s0 + u * THREADS];
        reduce(s0 + u * THREADS, [&](int j) __attribute__((always_inline)) {
          return la + qlen[j] - 2 * query_lcs<KIND>(V[u], j, qlen[j]);
        });
      }
    }
  }
  if (held >= 0) flush();
}

// The k closest options of every query (see "Fourth family" in the file
// header).  A wave's list of one query: lane r holds the key of rank r,
// ascending, ~0 = no entry.  Everything below runs with all 64 lanes active.
constexpr int K_MAX = 64;  // one rank per lane

__device__ __forceinline__ u64 readlane64(u64 v, int lane) {
  return ((u64)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), lane) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}

// Lane r gets lane r-1's value, lane 0 gets 0: v_mov_b32_dpp wave_shr:1 per
// half, no LDS crossbar.  (0x138 = wave_shr:1; with bound_ctrl off the lane
// without a source keeps `old`.)
__device__ __forceinline__ u64 wave_shr1(u64 v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v >> 32), 0x138, 0xf, 0xf, false);
  return ((u64)hi << 32) | lo;
}

// The wave-uniform key x goes into the list, the last rank falls out.  Keys
// are distinct (the option index is part of them), so a lane keeps its entry
// when it is smaller than x, takes x when its lower neighbour is smaller, and
// its lower neighbour's entry otherwise.
__device__ __forceinline__ void topk_insert(u64 &l, u64 x) {
  const u64 prev = wave_shr1(l);
  l = l < x ? l : (prev < x ? x : prev);
}

// Offer the keys of the lanes in `cand` (the ballot of key < tau) to the list:
// a scalar loop over the set bits.  tau, the key at rank k-1 = km1, is
// refreshed after every insertion and the remaining candidates are balloted
// against it again, so every pass of the loop is an insertion: an empty list
// with k = 1 takes about ln 64 of them from 64 candidates, not 64 tests.
__device__ __forceinline__ void topk_offer(u64 &l, u64 &tau, u64 key, u64 cand, int km1) {
  while (cand) {
    topk_insert(l, readlane64(key, __builtin_ctzll(cand)));
    tau = readlane64(l, km1);
    cand &= (cand - 1) & __builtin_amdgcn_ballot_w64(key < tau);
  }
}

// Work split and panel walk as in ed_closest_grouped_kernel; wave p of the
// launch's gridDim.x * 4 (workgroup-major) leaves its ranks 0 .. k-1 of the
// query in slot j of tile t at part[((t * NQ + j) * P + p) * k + rank], t
// counted from the launch's first tile.
template <int KIND, bool SCALED, int METRIC>
__global__ __launch_bounds__(THREADS) void ed_topk_kernel(
    const uint4 *__restrict__ panels, const int64_t *__restrict__ panelOff, const int *__restrict__ panelBlocks,
    const int *__restrict__ lenSorted, const int *__restrict__ perm, const uint4 *__restrict__ tileM,
    const int *__restrict__ tileQ, const int *__restrict__ tileLen, int nPanels, int k, u64 *__restrict__ part) {
  typedef TileT<KIND> TT;
  __shared__ uint4 T[TT::TABLE_U4];
  const int tile = blockIdx.y;
  load_tile<KIND>(tileM, tile, T);
  const int km1 = k - 1;
  int qlen[TT::NQ];
  u64 list[TT::NQ], tau[TT::NQ];  // tau[j]: wave-uniform, the key at rank k-1 (an empty query slot admits nothing)
#pragma unroll
  for (int j = 0; j < TT::NQ; j++) {
    qlen[j] = tileLen[tile * kTileSlots + j];
    list[j] = ~0ULL;
    tau[j] = tileQ[tile * kTileSlots + j] >= 0 ? ~0ULL : 0ULL;
  }

  // Slot s of this lane (empty: key ~0, which passes no bound), dist(j) = its
  // distance to query j.  Every branch is on a ballot or on tau: scalar.
  auto select = [&](int s, auto dist) __attribute__((always_inline)) {
    const int o = perm[s];
    u64 key[TT::NQ];
    bool any = false;
#pragma unroll
    for (int j = 0; j < TT::NQ; j++) {
      key[j] = o >= 0 ? ((u64)(unsigned)dist(j) << 32) | (unsigned)o : ~0ULL;
      any |= key[j] < tau[j];
    }
    if (__builtin_amdgcn_ballot_w64(any) == 0) return;  // the steady state
#pragma unroll
    for (int j = 0; j < TT::NQ; j++)
      topk_offer(list[j], tau[j], key[j], __builtin_amdgcn_ballot_w64(key[j] < tau[j]), km1);
  };

  for (int p = remap_panel(blockIdx.x, gridDim.x); p < nPanels; p += gridDim.x) {
    const int s0 = p * SLOTS + threadIdx.x;
    if constexpr (METRIC == METRIC_LEVENSHTEIN) {
      int la[OPT_PER_THREAD];
#pragma unroll
      for (int u = 0; u < OPT_PER_THREAD; u++) la[u] = lenSorted[s0 + u * THREADS];
      LevColumn<KIND> C[OPT_PER_THREAD];
      panel_lev<KIND, SCALED>(panels + panelOff[p], panelBlocks[p], reinterpret_cast<const char *>(T), la, C);
#pragma unroll
      for (int u = 0; u < OPT_PER_THREAD; u++)
        select(s0 + u * THREADS,
               [&](int j) __attribute__((always_inline)) { return query_lev<KIND>(C[u], j, qlen[j], la[u]); });
    } else {
      typename TT::W V[OPT_PER_THREAD][TT::NW];
      panel_lcs<KIND, SCALED>(panels + panelOff[p], panelBlocks[p], reinterpret_cast<const char *>(T), V);
#pragma unroll
      for (int u = 0; u < OPT_PER_THREAD; u++) {
        const int la = lenSorted[s0 + u * THREADS];
        select(s0 + u * THREADS, [&](int j) __attribute__((always_inline)) {
          return la + qlen[j] - 2 * query_lcs<KIND>(V[u], j, qlen[j]);
        });
      }
    }
  }

  const int lane = threadIdx.x & 63;
  const size_t P = (size_t)gridDim.x * (THREADS / 64), p = (size_t)blockIdx.x * (THREADS / 64) + threadIdx.x / 64;
#pragma unroll
  for (int j = 0; j < TT::NQ; j++)
    if (lane < k && tileQ[tile * kTileSlots + j] >= 0) part[(((size_t)tile * TT::NQ + j) * P + p) * k + lane] = list[j];
}

// One wave per query slot of one class (slot w = tile w / nq, query w % nq of
// the class's tiles): the P partial lists of k keys each, read 64 keys at a
// time, go through the same filter and insertion, and ranks 0 .. k-1 land in
// best[query * k + rank].  A key still ~0 passes no bound.
__global__ __launch_bounds__(THREADS) void ed_topk_merge_kernel(const u64 *__restrict__ part,
                                                                const int *__restrict__ tileQ, int nq, int slots,
                                                                int P, int k, u64 *__restrict__ best) {
  const int w = blockIdx.x * (THREADS / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
  if (w >= slots) return;  // whole waves leave
  const int q = tileQ[(w / nq) * kTileSlots + w % nq];
  if (q < 0) return;
  const size_t n = (size_t)P * k;
  const u64 *src = part + (size_t)w * n;
  u64 list = ~0ULL, tau = ~0ULL;
  for (size_t at = 0; at < n; at += 64) {
    const u64 key = at + lane < n ? src[at + lane] : ~0ULL;
    topk_offer(list, tau, key, __builtin_amdgcn_ballot_w64(key < tau), k - 1);
  }
  if (lane < k) best[(size_t)q * k + lane] = list;
}

// Many names against a few options (see "Fifth family" in the file header): the
// names sit in the panels, two to a lane, the options in the tiles.  The grid
// is over panels only; a workgroup walks the launch's tiles (one class, ordered
// by group) for every panel of its own, kNamesChunkBytes of tables resident in
// LDS at a time, and a lane keeps its two names' running minima in registers:
//   best[name * nGroups + g] = min over the options of group g of
//                              (dist << 32 | original option index)
// `t`, tileGroup[t], tileQ / tileLen[t] and `held` depend on kernel arguments
// and uniform loads only: they live in SGPRs and every branch on them is scalar.
constexpr int kNamesChunkBytes = 32 * 1024;

template <int KIND, bool SCALED, int METRIC>
__global__ __launch_bounds__(THREADS) void ed_closest_names_kernel(
    const uint4 *__restrict__ panels, const int64_t *__restrict__ panelOff, const int *__restrict__ panelBlocks,
    const int *__restrict__ lenSorted, const int *__restrict__ perm, const uint4 *__restrict__ tileM,
    const int *__restrict__ tileQ, const int *__restrict__ tileLen, const int *__restrict__ tileGroup, int nTiles,
    int nPanels, int nGroups, u64 *best) {
  typedef TileT<KIND> TT;
  constexpr int CHUNK = kNamesChunkBytes / TT::TABLE_BYTES;  // tiles resident at once: 8, the wide classes 4
  __shared__ uint4 T[CHUNK * TT::TABLE_U4];
  // Tables of tiles [first, first + n) of the launch into T, n <= CHUNK.
  auto stage = [&](int first, int n) __attribute__((always_inline)) {
    const uint4 *src = tileM + (size_t)first * TT::TABLE_U4;
    for (int i = threadIdx.x; i < n * TT::TABLE_U4; i += THREADS) T[i] = src[i];
    __syncthreads();
  };
  const bool resident = nTiles <= CHUNK;  // the expected case: staged once, before the panel walk
  if (resident) stage(0, nTiles);

  for (int p = remap_panel(blockIdx.x, gridDim.x); p < nPanels; p += gridDim.x) {
    const int s0 = p * SLOTS + threadIdx.x;
    int la[OPT_PER_THREAD], name[OPT_PER_THREAD];  // an empty slot: length 0, name -1, it commits nothing
    u64 key[OPT_PER_THREAD];
#pragma unroll
    for (int u = 0; u < OPT_PER_THREAD; u++) {
      la[u] = lenSorted[s0 + u * THREADS];
      name[u] = perm[s0 + u * THREADS];
      key[u] = ~0ULL;
    }
    const uint4 *panel = panels + panelOff[p];
    const int blocks = panelBlocks[p];
    int held = -1;  // the group of what key[] holds; -1 = nothing
    // One lane of one workgroup owns best[name][*], and the launches of a
    // request are ordered on its stream: a plain load / min / store.
    auto commit = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int u = 0; u < OPT_PER_THREAD; u++) {
        if (name[u] >= 0 && key[u] != ~0ULL) {
          u64 *b = best + (size_t)name[u] * nGroups + held;
          if (key[u] < *b) *b = key[u];
        }
        key[u] = ~0ULL;
      }
    };

    for (int c0 = 0; c0 < nTiles; c0 += CHUNK) {
      const int n = nTiles - c0 < CHUNK ? nTiles - c0 : CHUNK;
      if (!resident) {
        __syncthreads();  // every wave is done with the chunk before
        stage(c0, n);
      }
      for (int i = 0; i < n; i++) {
        const int t = c0 + i;
        const int g = tileGroup[t];
        if (g != held) {
          if (held >= 0) commit();
          held = g;
        }
        const char *Tt = reinterpret_cast<const char *>(T) + i * TT::TABLE_BYTES;
        const int *qid = tileQ + t * kTileSlots, *qlen = tileLen + t * kTileSlots;
        if constexpr (METRIC == METRIC_LEVENSHTEIN) {
          LevColumn<KIND> C[OPT_PER_THREAD];
          panel_lev<KIND, SCALED>(panel, blocks, Tt, la, C);
#pragma unroll
          for (int j = 0; j < TT::NQ; j++) {
            if (qid[j] < 0) continue;
#pragma unroll
            for (int u = 0; u < OPT_PER_THREAD; u++) {
              const u64 k = ((u64)(unsigned)query_lev<KIND>(C[u], j, qlen[j], la[u]) << 32) | (unsigned)qid[j];
              key[u] = k < key[u] ? k : key[u];
            }
          }
        } else {
          typename TT::W V[OPT_PER_THREAD][TT::NW];
          panel_lcs<KIND, SCALED>(panel, blocks, Tt, V);
#pragma unroll
          for (int j = 0; j < TT::NQ; j++) {
            if (qid[j] < 0) continue;
#pragma unroll
            for (int u = 0; u < OPT_PER_THREAD; u++) {
              const int d = la[u] + qlen[j] - 2 * query_lcs<KIND>(V[u], j, qlen[j]);
              const u64 k = ((u64)(unsigned)d << 32) | (unsigned)qid[j];
              key[u] = k < key[u] ? k : key[u];
            }
          }
        }
      }
    }
    if (held >= 0) commit();
  }
}

// Panel fill on the device (the normalising mode): raw option bytes in, the
// panels as [block][slot] 16-byte blocks of stored codes and lenSorted out,
// under a 256-entry byte map built by the host.  Entry 0 = drop the byte, any
// other entry = the stored code (code*4: this mode always runs the SCALED
// kernels); bytes that normalise to the same symbol share an entry, so what
// the normalisation is lies in the map and not in this code.
//  * Work split.  One lane per panel slot: SLOTS / THREADS workgroups per
//    panel, grid x = nPanels * SLOTS / THREADS.  Lane s of panel p fills slot
//    p*SLOTS + s from option perm[slot] (raw bytes offA[o] .. offA[o+1]).
//  * Byte map.  Staged in LDS once per workgroup by one coalesced dword load
//    of 64 lanes; a byte costs one ds_read_u8.
//  * Loads.  Aligned global_load_dwordx4 from the 16-byte block that holds the
//    option's first byte to the one that holds its last; bytes before the head
//    and after the tail are masked by index.  `raw` is 256-byte aligned and
//    its region a multiple of 256 bytes, so no lane reads outside it.  Lanes
//    of one panel have similar raw lengths (the options are sorted by it), so
//    the loop is balanced; their addresses are scattered over the raw region.
//  * Registers.  Kept codes are shifted into a word, full words into a 4-word
//    shift register (x <- y <- z <- w <- word): after four pushes the block is
//    in memory order without a dynamically indexed register array.
//  * Stores.  Every block is one uint4 to panels[panelOff[p] + b*SLOTS + s]:
//    consecutive lanes write consecutive 16 bytes.  After the last byte the
//    partial block goes out zero-padded, then zero blocks up to
//    panelBlocks[p]: the arena is reused between requests and nothing else
//    clears the panels, and code 0 leaves every column unchanged.  The host
//    plans panelBlocks from raw lengths, an upper bound on what a lane keeps.
//  * An empty slot (perm < 0) writes zero blocks and length 0.
// As compiled (hipcc -O3, gfx950, read from -save-temps): 22 VGPRs, 25 SGPRs,
// 256 bytes of LDS, no scratch; per 16 raw bytes one global_load_dwordx4 and 16
// ds_read_u8; every panel store is a global_store_dwordx4 (the only
// global_store_dword is lenSorted).  The 20 matcher kernels keep their VGPR,
// SGPR and LDS figures and stay without scratch.
__global__ __launch_bounds__(THREADS) void ed_fill_panels_kernel(
    const uint4 *__restrict__ raw, const int64_t *__restrict__ offA, const int *__restrict__ perm,
    const int64_t *__restrict__ panelOff, const int *__restrict__ panelBlocks, const uint32_t *__restrict__ byteMap,
    uint4 *__restrict__ panels, int *__restrict__ lenSorted) {
  __shared__ uint32_t mapWords[256 / sizeof(uint32_t)];
  if (threadIdx.x < 256 / sizeof(uint32_t)) mapWords[threadIdx.x] = byteMap[threadIdx.x];
  __syncthreads();
  const uint8_t *map = reinterpret_cast<const uint8_t *>(mapWords);

  const int p = blockIdx.x / (SLOTS / THREADS);
  const int s = (blockIdx.x % (SLOTS / THREADS)) * THREADS + threadIdx.x;
  const int slot = p * SLOTS + s;
  const int blocks = panelBlocks[p];
  uint4 *dst = panels + panelOff[p] + s;
  const int o = perm[slot];

  uint4 blk = make_uint4(0, 0, 0, 0);
  uint32_t word = 0;
  int kept = 0;  // codes kept so far: byte kept%4 of word kept/4%4 of block kept/16 is next
  auto push_word = [&]() __attribute__((always_inline)) {
    blk.x = blk.y;
    blk.y = blk.z;
    blk.z = blk.w;
    blk.w = word;
    word = 0;
  };
  auto store_block = [&](int b) __attribute__((always_inline)) {
    if (b < blocks) dst[(size_t)b * SLOTS] = blk;
  };
  if (o >= 0) {
    const int64_t beg = offA[o], end = offA[o + 1];
    const int64_t first = beg >> 4;  // the option's first 16-byte block of `raw`
    const int lo = (int)(beg - (first << 4)), hi = (int)(end - (first << 4));
    const uint4 *src = raw + first;
    for (int at = 0; at < hi; at += 16) {  // nothing is loaded for an empty option
      const uint4 q = *src++;
      const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const uint32_t c = map[(w4[i / 4] >> (8 * (i % 4))) & 0xffu];
        if (at + i >= lo && at + i < hi && c != 0) {
          word |= c << (8 * (kept & 3));
          kept++;
          if ((kept & 3) == 0) {
            push_word();
            if ((kept & 15) == 0) store_block(kept / 16 - 1);
          }
        }
      }
    }
  }
  int b = kept / 16;
  if (kept & 15) {  // the partial block: its words so far, the partial word, zero words
    for (int w = (kept & 15) / 4; w < 4; w++) push_word();
    store_block(b++);
  }
  // (the loop vectoriser would pair these and split every block into four dword stores)
#pragma clang loop vectorize(disable) interleave(disable)
  for (; b < blocks; b++) dst[(size_t)b * SLOTS] = make_uint4(0, 0, 0, 0);
  lenSorted[slot] = kept;
}

// ---------------------------------------------------------------------------
// Host side.  One request = code map + length sort + panel fill, written
// straight into a pinned staging buffer that is laid out exactly like the
// device buffer, then ONE async H2D copy, the kernels and the D2H of the
// results on one stream.  Staging/device buffers and the stream live in a
// grow-only per-process arena (no hipMalloc/hipFree/hipHostMalloc per call;
// hipFree would also serialise the device).  The fill runs on host threads;
// in a normalising mode (raw names in, see prepare_norm) the raw option bytes
// are copied instead and ed_fill_panels_kernel fills the panels on the device.
// ---------------------------------------------------------------------------
namespace {

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int host_threads() {
  unsigned h = std::thread::hardware_concurrency();
  int t = h ? (int)h : 4;
  if (const char *e = getenv("M2K_ED_THREADS")) t = atoi(e);
  return std::max(1, std::min(t, 32));
}

// f(lo, hi) over [0, n) in nt contiguous chunks
template <class F>
void par_for(int64_t n, int nt, int64_t grain, F f) {
  if (n <= 0) return;
  if (nt <= 1 || n < 2 * grain) {
    f(0, n);
    return;
  }
  nt = (int)std::min<int64_t>(nt, (n + grain - 1) / grain);
  std::vector<std::thread> pool;
  const int64_t chunk = (n + nt - 1) / nt;
  for (int t = 1; t < nt; t++) {
    const int64_t lo = t * chunk, hi = std::min(n, lo + chunk);
    if (lo < hi) pool.emplace_back(f, lo, hi);
  }
  f(0, std::min(n, chunk));
  for (auto &th : pool) th.join();
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

#define PER_KIND(F) {TileT<K16>::F, TileT<K32>::F, TileT<K64>::F, TileT<K128>::F, TileT<K256>::F}
const int kKindMaxLen[NKINDS] = PER_KIND(MAXLEN);
const int kKindQueries[NKINDS] = PER_KIND(NQ);
const size_t kKindTableBytes[NKINDS] = PER_KIND(TABLE_BYTES);
#undef PER_KIND
const int kMaxQueryBytes = TileT<NKINDS - 1>::MAXLEN;

// Offsets into the staging/device buffer.  Tile kinds are contiguous runs of
// tiles in length order, and so are their tables.
struct Layout {
  int nA = 0, nB = 0, nPanels = 0, scaled = 0;
  int nGroups = 0;  // > 0: a grouped request (groupSorted is laid out, `best` holds nB * nGroups keys)
  int k = 0;        // > 0: a top-k request (`best` holds nB * k keys, the part plan below is set)
  int names = 0;    // the names route: nA names in the panels, nB options in the tiles, grouped by tileGroup
                    // (nGroups >= 1, no groupSorted), `best` holds nA * nGroups keys
  int nTiles = 0, kindStart[NKINDS] = {0, 0, 0, 0, 0}, kindCount[NKINDS] = {0, 0, 0, 0, 0};
  size_t oPanels = 0, oPanelOff = 0, oPanelBlocks = 0, oLenSorted = 0, oPerm = 0, oTileQ = 0, oTileLen = 0;
  size_t kindTableOff[NKINDS] = {0, 0, 0, 0, 0};  // the tables of the kind's first tile
  size_t oRaw = 0, oOffA = 0, oByteMap = 0;       // device fill only: its input
  size_t oGroup = 0;                               // grouped requests only: groupSorted
  size_t oTileGroup = 0;                           // names route only: tileGroup
  size_t h2dBytes = 0, oBest = 0, bytes = 0;
  // Top-k only, in u64 keys of the device-only partial buffer (Arena::out): a class's tiles write partCount =
  // 4 * gridDim.x lists of k keys per query slot, from partOff on, tile-major.
  size_t partOff[NKINDS] = {0, 0, 0, 0, 0}, partKeys = 0;
  int partCount[NKINDS] = {0, 0, 0, 0, 0};
  size_t nBest() const { return names ? (size_t)nA * nGroups : (size_t)nB * (size_t)(k > 0 ? k : std::max(nGroups, 1)); }

  // Byte offset of the mask tables of a tile of `kind`.
  size_t tileTable(int kind, int tile) const {
    return kindTableOff[kind] + kKindTableBytes[kind] * (size_t)(tile - kindStart[kind]);
  }
};

struct Arena {
  std::mutex mu;
  char *host = nullptr;  // pinned staging, same layout as dev
  char *dev = nullptr;
  size_t cap = 0;
  int *out = nullptr;  // ed_matrix output; the partial lists of a top-k request
  size_t outCap = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  double last[5] = {0, 0, 0, 0, 0};  // prep, h2d, kernel, d2h, fill (ms)

  int ensure(size_t bytes) {
    if (!stream) {
      if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return -4;
      for (auto &e : ev)
        if (hipEventCreate(&e) != hipSuccess) return -4;
    }
    if (bytes <= cap) return 0;
    const size_t want = std::max(bytes, cap + cap / 2);
    if (host) (void)hipHostFree(host);
    if (dev) (void)hipFree(dev);
    host = dev = nullptr;
    cap = 0;
    if (hipHostMalloc(reinterpret_cast<void **>(&host), want, hipHostMallocDefault) != hipSuccess) return -4;
    if (hipMalloc(reinterpret_cast<void **>(&dev), want) != hipSuccess) return -4;
    cap = want;
    return 0;
  }
  int ensure_out(size_t bytes) {
    if (bytes <= outCap) return 0;
    if (out) (void)hipFree(out);
    out = nullptr;
    outCap = 0;
    if (hipMalloc(reinterpret_cast<void **>(&out), bytes) != hipSuccess) return -4;
    outCap = bytes;
    return 0;
  }
};

// Process lifetime on purpose: destroying HIP objects from a static destructor
// races the runtime's own teardown.
Arena &arena() {
  static Arena *a = new Arena();
  return *a;
}

// Dense codes ranked by option-byte frequency; 0 is reserved for padding.
// Returns false when all 256 byte values occur (no free code for padding).
// The counting pass: freq[b] = how often byte b occurs in the options.
void count_bytes(const uint8_t *opts, int64_t nOptBytes, int nt, int64_t freq[256]) {
  std::vector<std::array<int64_t, 256>> part(std::max(1, nt));
  for (auto &p : part) p.fill(0);
  std::atomic<int> slot{0};
  par_for(nOptBytes, nt, 1 << 20, [&](int64_t lo, int64_t hi) {
    auto &f = part[slot.fetch_add(1)];
    for (int64_t i = lo; i < hi; i++) f[opts[i]]++;
  });
  std::fill(freq, freq + 256, 0);
  for (auto &p : part)
    for (int b = 0; b < 256; b++) freq[b] += p[b];
}

// The ranking: a code for every symbol that occurs in the options (freq > 0)
// or the queries, most frequent option symbol first.
bool rank_codes(const int64_t freq[256], const uint8_t *qs, int64_t nQBytes, uint8_t code[256], int *nsym) {
  bool seen[256] = {false};
  for (int b = 0; b < 256; b++) seen[b] = freq[b] > 0;
  for (int64_t i = 0; i < nQBytes; i++) seen[qs[i]] = true;
  int order[256];
  int n = 0;
  for (int b = 0; b < 256; b++)
    if (seen[b]) order[n++] = b;
  if (n > 255) return false;
  std::stable_sort(order, order + n, [&](int x, int y) { return freq[x] > freq[y]; });
  memset(code, 0, 256);
  for (int i = 0; i < n; i++) code[order[i]] = (uint8_t)(i + 1);
  *nsym = n;
  return true;
}

bool build_code_map(const uint8_t *opts, int64_t nOptBytes, const uint8_t *qs, int64_t nQBytes, int nt,
                    uint8_t code[256], int *nsym) {
  int64_t freq[256];
  count_bytes(opts, nOptBytes, nt, freq);
  return rank_codes(freq, qs, nQBytes, code, nsym);
}

// Normalising modes of run(): what a raw byte becomes before it is matched.
// A mode is a 256-entry table, 0 = the byte is dropped, anything else = the
// symbol it stands for.  ALNUM_LOWER is the matcher's caller's
// lower(strip([^a-zA-Z0-9]+)) on UTF-8 bytes: every byte of a non-ASCII rune
// is >= 0x80 and goes with the separators, so no rune is ever decoded.
enum { MODE_NONE = 0, MODE_ALNUM_LOWER = 1 };

void symbol_table(int mode, uint8_t sym[256]) {
  memset(sym, 0, 256);
  if (mode == MODE_ALNUM_LOWER) {
    for (int b = '0'; b <= '9'; b++) sym[b] = (uint8_t)b;
    for (int b = 'a'; b <= 'z'; b++) sym[b] = sym[b - 'a' + 'A'] = (uint8_t)b;
  }
}

bool query_lengths_ok(const int64_t *offB, int nB) {
  for (int j = 0; j < nB; j++) {
    const int64_t len = offB[j + 1] - offB[j];
    if (len < 0 || len > kMaxQueryBytes) return false;
  }
  return true;
}

// Options in length order (stable), cut into panels of SLOTS: blocks[p] =
// 16-byte blocks of panel p, off[p] = its first uint4 (off[nPanels] = total).
struct PanelPlan {
  std::vector<int> order, blocks;
  std::vector<int64_t> off;
};

// With groups (groupOf set, nGroups > 1) the order is (group, length), stable:
// groups share panels, and a panel's longest option need not be its last.
PanelPlan plan_panels(const int64_t *offA, int nA, const int32_t *groupOf = nullptr, int nGroups = 0) {
  PanelPlan P;
  // stable counting sort of the options by length
  int maxLen = 0;
  for (int i = 0; i < nA; i++) maxLen = std::max(maxLen, (int)(offA[i + 1] - offA[i]));
  P.order.resize(nA);
  if (maxLen <= (1 << 20)) {
    std::vector<int> start(maxLen + 2, 0);
    for (int i = 0; i < nA; i++) start[(int)(offA[i + 1] - offA[i]) + 1]++;
    for (int l = 0; l <= maxLen; l++) start[l + 1] += start[l];
    for (int i = 0; i < nA; i++) P.order[start[(int)(offA[i + 1] - offA[i])]++] = i;
  } else {
    std::iota(P.order.begin(), P.order.end(), 0);
    std::stable_sort(P.order.begin(), P.order.end(),
                     [&](int x, int y) { return (offA[x + 1] - offA[x]) < (offA[y + 1] - offA[y]); });
  }
  const bool grouped = groupOf && nGroups > 1;
  if (grouped) {  // a second stable counting pass, by group, keeps the length order within a group
    std::vector<int> byLen(P.order), start(nGroups + 1, 0);
    for (int i = 0; i < nA; i++) start[groupOf[i] + 1]++;
    for (int g = 0; g < nGroups; g++) start[g + 1] += start[g];
    for (int i = 0; i < nA; i++) P.order[start[groupOf[byLen[i]]]++] = byLen[i];
  }
  const int nPanels = (nA + SLOTS - 1) / SLOTS;
  P.blocks.resize(nPanels);
  P.off.resize(nPanels + 1);
  int64_t total = 0;
  for (int p = 0; p < nPanels; p++) {
    const int last = std::min(nA, (p + 1) * SLOTS) - 1;  // sorted by length alone: the panel's longest option
    int64_t longest = 0;
    for (int k = grouped ? p * SLOTS : last; k <= last; k++)
      longest = std::max(longest, offA[P.order[k] + 1] - offA[P.order[k]]);
    P.blocks[p] = (int)((longest + 15) / 16);
    P.off[p] = total;
    total += (int64_t)P.blocks[p] * SLOTS;
  }
  P.off[nPanels] = total;
  return P;
}

// Query tiles: the queries in length order, each in the first class whose
// MAXLEN holds it, NQ of them to a tile.  q / len are the tileQ / tileLen rows
// (kTileSlots per tile); kindStart / kindCount get each class's run of tiles.
struct TilePlan {
  std::vector<int> q, len;
  std::vector<int> group;  // names route only: tileGroup[t]
};

TilePlan plan_tiles(const int64_t *offB, int nB, int kindStart[NKINDS], int kindCount[NKINDS]) {
  std::vector<int> qorder(nB);
  {
    int start[kMaxQueryBytes + 2] = {0};
    for (int j = 0; j < nB; j++) start[(int)(offB[j + 1] - offB[j]) + 1]++;
    for (int l = 0; l <= kMaxQueryBytes; l++) start[l + 1] += start[l];
    for (int j = 0; j < nB; j++) qorder[start[(int)(offB[j + 1] - offB[j])]++] = j;
  }
  TilePlan P;
  int kindOfPrev = -1, fill = 0;
  for (int r = 0; r < nB; r++) {
    const int j = qorder[r];
    const int len = (int)(offB[j + 1] - offB[j]);
    int kind = K16;
    while (len > kKindMaxLen[kind]) kind++;
    if (kind != kindOfPrev || fill == kKindQueries[kind]) {
      if (kind != kindOfPrev) kindStart[kind] = (int)(P.q.size() / kTileSlots);
      P.q.insert(P.q.end(), kTileSlots, -1);
      P.len.insert(P.len.end(), kTileSlots, 0);
      kindCount[kind]++;
      kindOfPrev = kind;
      fill = 0;
    }
    P.q[P.q.size() - kTileSlots + fill] = j;
    P.len[P.len.size() - kTileSlots + fill] = len;
    fill++;
  }
  return P;
}

// The names route's tiles: the options (the tile side there) ordered by (class,
// group, length), stable, so a class's tiles are one run and a group's tiles
// one run within it.  A tile never holds two groups: it is closed on a change
// of class or group and its remaining slots stay empty (-1, length 0).
// groupOf == nullptr: one group.
TilePlan plan_tiles_grouped(const int64_t *offB, int nB, const int32_t *groupOf, int kindStart[NKINDS],
                            int kindCount[NKINDS]) {
  auto length = [&](int j) { return (int)(offB[j + 1] - offB[j]); };
  auto kindOf = [&](int j) {
    int kind = K16;
    while (length(j) > kKindMaxLen[kind]) kind++;
    return kind;
  };
  std::vector<int> order(nB);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
    const int kx = kindOf(x), ky = kindOf(y), gx = groupOf ? groupOf[x] : 0, gy = groupOf ? groupOf[y] : 0;
    if (kx != ky) return kx < ky;
    if (gx != gy) return gx < gy;
    return length(x) < length(y);
  });
  TilePlan P;
  int kindOfPrev = -1, groupOfPrev = -1, fill = 0;
  for (int r = 0; r < nB; r++) {
    const int j = order[r], kind = kindOf(j), g = groupOf ? groupOf[j] : 0;
    if (kind != kindOfPrev || g != groupOfPrev || fill == kKindQueries[kind]) {
      if (kind != kindOfPrev) kindStart[kind] = (int)P.group.size();
      P.q.insert(P.q.end(), kTileSlots, -1);
      P.len.insert(P.len.end(), kTileSlots, 0);
      P.group.push_back(g);
      kindCount[kind]++;
      kindOfPrev = kind;
      groupOfPrev = g;
      fill = 0;
    }
    P.q[P.q.size() - kTileSlots + fill] = j;
    P.len[P.len.size() - kTileSlots + fill] = length(j);
    fill++;
  }
  return P;
}

// Offsets of every array in the staging/device buffer; needs L's panel and tile counts.
// rawBytes < 0: the host fills the panels and everything up to the tables is
// copied.  rawBytes >= 0: the device fills them from the raw option bytes, so
// the copied range ends with the fill kernel's input (option offsets, byte
// map, raw bytes; every region 256-byte aligned and a multiple of 256 bytes)
// and the panels and lenSorted lie behind it.
int grid_x(int nPanels, int tiles);

void lay_out(Layout &L, int64_t panelU4, int64_t rawBytes = -1) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o = align256(o + bytes);
    return at;
  };
  const bool deviceFill = rawBytes >= 0;
  const size_t panelBytes = sizeof(uint4) * (size_t)std::max<int64_t>(panelU4, 1);
  const size_t lenBytes = sizeof(int) * (size_t)L.nPanels * SLOTS;
  if (!deviceFill) L.oPanels = take(panelBytes);
  L.oPanelOff = take(sizeof(int64_t) * (size_t)(L.nPanels + 1));
  L.oPanelBlocks = take(sizeof(int) * (size_t)L.nPanels);
  if (!deviceFill) L.oLenSorted = take(lenBytes);
  L.oPerm = take(sizeof(int) * (size_t)L.nPanels * SLOTS);
  if (L.nGroups > 0 && !L.names) L.oGroup = take(sizeof(int) * (size_t)L.nPanels * SLOTS);
  if (L.names) L.oTileGroup = take(sizeof(int) * (size_t)L.nTiles);
  L.oTileQ = take(sizeof(int) * (size_t)L.nTiles * kTileSlots);
  L.oTileLen = take(sizeof(int) * (size_t)L.nTiles * kTileSlots);
  for (int k = 0; k < NKINDS; k++) L.kindTableOff[k] = take(kKindTableBytes[k] * (size_t)L.kindCount[k]);
  if (deviceFill) {
    L.oOffA = take(sizeof(int64_t) * (size_t)(L.nA + 1));
    L.oByteMap = take(256);
    L.oRaw = take((size_t)rawBytes);
  }
  L.h2dBytes = o;
  if (deviceFill) {
    L.oPanels = take(panelBytes);
    L.oLenSorted = take(lenBytes);
  }
  L.oBest = take(sizeof(u64) * L.nBest());
  L.bytes = o;
  if (L.k > 0)  // the part plan: launch_kind gives a class's tiles grid_x workgroups of 4 waves
    for (int kind = 0; kind < NKINDS; kind++) {
      if (L.kindCount[kind] == 0) continue;
      L.partCount[kind] = (THREADS / 64) * grid_x(L.nPanels, L.kindCount[kind]);
      L.partOff[kind] = L.partKeys;
      L.partKeys += (size_t)L.kindCount[kind] * kKindQueries[kind] * L.partCount[kind] * L.k;
    }
}

// Panels as 16-byte blocks [block][slot] of stored codes, padded with code 0;
// perm / lenSorted = each slot's original option index (-1 = none) and length.
void fill_panels(const uint8_t *opts, const int64_t *offA, int nA, const PanelPlan &P, const uint8_t (&stored)[256],
                 int nt, uint4 *panels, int *perm, int *lenSorted) {
  par_for((int64_t)P.blocks.size(), nt, 4, [&](int64_t plo, int64_t phi) {
    for (int64_t p = plo; p < phi; p++) {
      uint8_t *base = reinterpret_cast<uint8_t *>(panels + P.off[p]);
      memset(base, 0, sizeof(uint4) * (size_t)P.blocks[p] * SLOTS);
      for (int s = 0; s < SLOTS; s++) {
        const int64_t k = p * SLOTS + s;
        if (k >= nA) {
          perm[k] = -1;
          lenSorted[k] = 0;
          continue;
        }
        const int opt = P.order[k];
        const uint8_t *src = opts + offA[opt];
        const int len = (int)(offA[opt + 1] - offA[opt]);
        perm[k] = opt;
        lenSorted[k] = len;
        for (int b = 0; b * 16 < len; b++) {
          uint8_t *dst = base + ((size_t)b * SLOTS + s) * 16;
          const int n = std::min(16, len - b * 16);
          for (int t = 0; t < n; t++) dst[t] = stored[src[b * 16 + t]];
        }
      }
    }
  });
}

// Mask tables of every tile.  Column-bit convention, the same for every class:
// the query in slot s owns bits [s*MAXLEN, (s+1)*MAXLEN) of the tile's column,
// so its byte k is column bit P = s*MAXLEN + k, and a match of code c there is
// bit P%64 of entry c of sub-table P/64 (step4 and query_lcs read it back as
// 16-bit halves, 32-bit words or u64 words of that one column).
void fill_tables(const uint8_t *qs, const int64_t *offB, const uint8_t (&code)[256], const TilePlan &tiles,
                 const Layout &L, int nt, char *h) {
  par_for(L.nTiles, nt, 32, [&](int64_t lo, int64_t hi) {
    for (int kind = 0; kind < NKINDS; kind++) {  // the part of [lo, hi) that is this kind's run
      const int64_t end = std::min<int64_t>(hi, L.kindStart[kind] + L.kindCount[kind]);
      for (int64_t t = std::max<int64_t>(lo, L.kindStart[kind]); t < end; t++) {
        u64 *T64 = reinterpret_cast<u64 *>(h + L.tileTable(kind, (int)t));
        memset(T64, 0, kKindTableBytes[kind]);
        for (int slot = 0; slot < kKindQueries[kind]; slot++) {
          const int j = tiles.q[t * kTileSlots + slot];
          if (j < 0) continue;
          const int len = tiles.len[t * kTileSlots + slot];
          for (int k = 0; k < len; k++) {
            const int c = code[qs[offB[j] + k]];
            const int P = slot * kKindMaxLen[kind] + k;
            T64[(P / 64) * kTableEntries + c] |= 1ULL << (P % 64);
          }
        }
      }
    }
  });
}

// groupSorted[slot] = the group of the slot's option, -1 for an empty slot.
void fill_groups(const PanelPlan &P, int nA, const int32_t *groupOf, const Layout &L, char *h) {
  int *groupSorted = reinterpret_cast<int *>(h + L.oGroup);
  for (int k = 0; k < nA; k++) groupSorted[k] = groupOf[P.order[k]];
  std::fill(groupSorted + nA, groupSorted + (size_t)L.nPanels * SLOTS, -1);
}

// Everything up to (not including) the H2D copy.  Returns 0 or an error code.
// `names`: the names route, where the panel side (opts) is the names, the tile
// side (qs) the options and groupOf the options' groups (nullptr: one group).
int prepare(const uint8_t *opts, const int64_t *offA, int nA, const int32_t *groupOf, int nGroups, const uint8_t *qs,
            const int64_t *offB, int nB, Arena &ar, Layout &L, bool names = false) {
  if (!query_lengths_ok(offB, nB)) return -2;
  const int nt = host_threads();
  uint8_t code[256];
  int nsym = 0;
  if (!build_code_map(opts, offA[nA], qs, offB[nB], nt, code, &nsym)) return -8;
  L.nA = nA;
  L.nB = nB;
  L.scaled = nsym <= 63;
  uint8_t stored[256];
  for (int b = 0; b < 256; b++) stored[b] = L.scaled ? (uint8_t)(code[b] * 4) : code[b];

  const PanelPlan panels = names ? plan_panels(offA, nA) : plan_panels(offA, nA, groupOf, nGroups);
  L.names = names;
  L.nGroups = names ? std::max(nGroups, 1) : groupOf ? nGroups : 0;
  L.nPanels = (int)panels.blocks.size();
  const TilePlan tiles = names ? plan_tiles_grouped(offB, nB, groupOf, L.kindStart, L.kindCount)
                               : plan_tiles(offB, nB, L.kindStart, L.kindCount);
  L.nTiles = (int)(tiles.q.size() / kTileSlots);
  lay_out(L, panels.off[L.nPanels]);
  if (int rc = ar.ensure(L.bytes)) return rc;

  char *h = ar.host;
  memcpy(h + L.oPanelOff, panels.off.data(), sizeof(int64_t) * panels.off.size());
  memcpy(h + L.oPanelBlocks, panels.blocks.data(), sizeof(int) * panels.blocks.size());
  if (L.nGroups > 0 && !names) fill_groups(panels, nA, groupOf, L, h);
  if (names) memcpy(h + L.oTileGroup, tiles.group.data(), sizeof(int) * tiles.group.size());
  fill_panels(opts, offA, nA, panels, stored, nt, reinterpret_cast<uint4 *>(h + L.oPanels),
              reinterpret_cast<int *>(h + L.oPerm), reinterpret_cast<int *>(h + L.oLenSorted));
  memcpy(h + L.oTileQ, tiles.q.data(), sizeof(int) * tiles.q.size());
  memcpy(h + L.oTileLen, tiles.len.data(), sizeof(int) * tiles.len.size());
  fill_tables(qs, offB, code, tiles, L, nt, h);
  return 0;
}

// prepare() of a normalising mode: the options go to the device as they are
// and ed_fill_panels_kernel does their per-byte work.  The host normalises the
// queries (few, and the tile plan needs their lengths), folds the raw byte
// counts through the mode's symbol table to rank the codes as prepare() does,
// and plans the panels on the raw lengths: an upper bound on the normalised
// ones, the surplus blocks hold code 0.  It reads the option bytes once, to
// count them, and copies them once.
int prepare_norm(const uint8_t *opts, const int64_t *offA, int nA, const int32_t *groupOf, int nGroups,
                 const uint8_t *qs, const int64_t *offB, int nB, int mode, Arena &ar, Layout &L, bool names = false) {
  uint8_t sym[256];
  symbol_table(mode, sym);
  std::vector<uint8_t> nq;
  std::vector<int64_t> nOffB(nB + 1, 0);
  nq.reserve((size_t)std::max<int64_t>(offB[nB], 0));
  for (int j = 0; j < nB; j++) {
    for (int64_t i = offB[j]; i < offB[j + 1]; i++)
      if (sym[qs[i]]) nq.push_back(sym[qs[i]]);
    nOffB[j + 1] = (int64_t)nq.size();
  }
  if (!query_lengths_ok(nOffB.data(), nB)) return -2;
  const int nt = host_threads();
  int64_t rawFreq[256], freq[256] = {0};
  count_bytes(opts, offA[nA], nt, rawFreq);
  for (int b = 0; b < 256; b++)
    if (sym[b]) freq[sym[b]] += rawFreq[b];
  uint8_t code[256];
  int nsym = 0;
  if (!rank_codes(freq, nq.data(), (int64_t)nq.size(), code, &nsym) || nsym > 63) return -8;  // 36 symbols: never
  L.nA = nA;
  L.nB = nB;
  L.scaled = 1;

  const PanelPlan panels = names ? plan_panels(offA, nA) : plan_panels(offA, nA, groupOf, nGroups);
  L.names = names;
  L.nGroups = names ? std::max(nGroups, 1) : groupOf ? nGroups : 0;
  L.nPanels = (int)panels.blocks.size();
  const TilePlan tiles = names ? plan_tiles_grouped(nOffB.data(), nB, groupOf, L.kindStart, L.kindCount)
                               : plan_tiles(nOffB.data(), nB, L.kindStart, L.kindCount);
  L.nTiles = (int)(tiles.q.size() / kTileSlots);
  lay_out(L, panels.off[L.nPanels], offA[nA]);
  if (int rc = ar.ensure(L.bytes)) return rc;

  char *h = ar.host;
  memcpy(h + L.oPanelOff, panels.off.data(), sizeof(int64_t) * panels.off.size());
  memcpy(h + L.oPanelBlocks, panels.blocks.data(), sizeof(int) * panels.blocks.size());
  if (L.nGroups > 0 && !names) fill_groups(panels, nA, groupOf, L, h);
  if (names) memcpy(h + L.oTileGroup, tiles.group.data(), sizeof(int) * tiles.group.size());
  int *perm = reinterpret_cast<int *>(h + L.oPerm);
  memcpy(perm, panels.order.data(), sizeof(int) * (size_t)nA);
  std::fill(perm + nA, perm + (size_t)L.nPanels * SLOTS, -1);
  memcpy(h + L.oTileQ, tiles.q.data(), sizeof(int) * tiles.q.size());
  memcpy(h + L.oTileLen, tiles.len.data(), sizeof(int) * tiles.len.size());
  fill_tables(nq.data(), nOffB.data(), code, tiles, L, nt, h);
  memcpy(h + L.oOffA, offA, sizeof(int64_t) * (size_t)(nA + 1));
  uint8_t *byteMap = reinterpret_cast<uint8_t *>(h + L.oByteMap);
  for (int b = 0; b < 256; b++) byteMap[b] = sym[b] ? (uint8_t)(code[sym[b]] * 4) : 0;
  memcpy(h + L.oRaw, opts, (size_t)offA[nA]);
  return 0;
}

int grid_x(int nPanels, int tiles) {
  // ~4k workgroups per launch: ~2 rounds of the 256 CUs x 7 resident 256-thread
  // groups, each walking enough panels to amortise staging its 4 KiB tile table
  // and the per-query reductions (16k tiny groups measured 3x slower for K16).
  // x is a multiple of 8 for the XCD remap.  The wide tiles keep the target:
  // a group stages 8 KiB but also does twice the work per panel, and 8 KiB of
  // LDS still leaves registers, not LDS, as what bounds the resident groups.
  static const int target = getenv("M2K_ED_WGS") ? std::max(1, atoi(getenv("M2K_ED_WGS"))) : 4096;
  int want = (target + tiles - 1) / tiles;
  want = std::max(8, std::min(want, 1024));
  int x = std::min(nPanels, want);
  if (x >= 8) x = (x / 8) * 8;
  return x < 1 ? 1 : x;
}

template <class T>
T *dev_at(const Arena &ar, size_t off) {
  return reinterpret_cast<T *>(ar.dev + off);
}

// The names route's grid: over panels alone.  Up to kNamesMaxGrid panels get a
// workgroup each (they differ in length, the hardware balances them, and
// staging <= 32 KiB of tables per workgroup is a few percent of one panel's
// work); beyond that the workgroups are persistent and stride, x a multiple of
// 8 for the XCD remap.
constexpr int kNamesMaxGrid = 4096;
int names_grid_x(int nPanels) { return nPanels <= kNamesMaxGrid ? std::max(nPanels, 1) : kNamesMaxGrid; }

// One class's tiles of a names request: one launch, the tile loop is the kernel's.
template <int KIND, bool SCALED, int METRIC>
int launch_names_kind(const Layout &L, const Arena &ar, hipStream_t s) {
  const int count = L.kindCount[KIND], tile0 = L.kindStart[KIND];
  if (count == 0) return 0;
  hipLaunchKernelGGL((ed_closest_names_kernel<KIND, SCALED, METRIC>), dim3(names_grid_x(L.nPanels)), dim3(THREADS), 0,
                     s, dev_at<const uint4>(ar, L.oPanels), dev_at<const int64_t>(ar, L.oPanelOff),
                     dev_at<const int>(ar, L.oPanelBlocks), dev_at<const int>(ar, L.oLenSorted),
                     dev_at<const int>(ar, L.oPerm), dev_at<const uint4>(ar, L.tileTable(KIND, tile0)),
                     dev_at<const int>(ar, L.oTileQ) + (size_t)tile0 * kTileSlots,
                     dev_at<const int>(ar, L.oTileLen) + (size_t)tile0 * kTileSlots,
                     dev_at<const int>(ar, L.oTileGroup) + tile0, count, L.nPanels, L.nGroups,
                     dev_at<u64>(ar, L.oBest));
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// One class's tiles: the matrix kernels when `out` is set, the grouped closest
// kernels for a grouped request, the top-k kernels for a top-k request (slab t
// writes its tiles' partial lists behind those of the slabs before it), the
// closest kernels otherwise.
template <int KIND, bool SCALED, int METRIC>
int launch_kind(const Layout &L, const Arena &ar, int *out, hipStream_t s) {
  if (L.names) return launch_names_kind<KIND, SCALED, METRIC>(L, ar, s);
  const int count = L.kindCount[KIND];
  if (count == 0) return 0;
  const int gx = grid_x(L.nPanels, count);
  const uint4 *panels = dev_at<uint4>(ar, L.oPanels);
  const int64_t *panelOff = dev_at<int64_t>(ar, L.oPanelOff);
  const int *panelBlocks = dev_at<int>(ar, L.oPanelBlocks), *lenSorted = dev_at<int>(ar, L.oLenSorted);
  const int *perm = dev_at<int>(ar, L.oPerm);
  for (int t = 0; t < count; t += MAX_Y) {
    const int rows = std::min(MAX_Y, count - t);
    // every launch gets its own first tile's tables and tileQ / tileLen rows
    const int tile0 = L.kindStart[KIND] + t;
    const uint4 *tileM = dev_at<uint4>(ar, L.tileTable(KIND, tile0));
    const int *tileQ = dev_at<int>(ar, L.oTileQ) + (size_t)tile0 * kTileSlots;
    const int *tileLen = dev_at<int>(ar, L.oTileLen) + (size_t)tile0 * kTileSlots;
    if (out)
      hipLaunchKernelGGL((ed_matrix_kernel<KIND, SCALED, METRIC>), dim3(gx, rows), dim3(THREADS), 0, s, panels, panelOff,
                         panelBlocks, lenSorted, perm, tileM, tileQ, tileLen, L.nA, L.nPanels, out);
    else if (L.nGroups > 0)
      hipLaunchKernelGGL((ed_closest_grouped_kernel<KIND, SCALED, METRIC>), dim3(gx, rows), dim3(THREADS), 0, s, panels,
                         panelOff, panelBlocks, lenSorted, perm, dev_at<int>(ar, L.oGroup), tileM, tileQ, tileLen,
                         L.nPanels, L.nGroups, dev_at<u64>(ar, L.oBest));
    else if (L.k > 0)
      hipLaunchKernelGGL((ed_topk_kernel<KIND, SCALED, METRIC>), dim3(gx, rows), dim3(THREADS), 0, s, panels, panelOff,
                         panelBlocks, lenSorted, perm, tileM, tileQ, tileLen, L.nPanels, L.k,
                         reinterpret_cast<u64 *>(ar.out) + L.partOff[KIND] +
                             (size_t)t * kKindQueries[KIND] * L.partCount[KIND] * L.k);
    else
      hipLaunchKernelGGL((ed_closest_kernel<KIND, SCALED, METRIC>), dim3(gx, rows), dim3(THREADS), 0, s, panels, panelOff,
                         panelBlocks, lenSorted, perm, tileM, tileQ, tileLen, L.nPanels, dev_at<u64>(ar, L.oBest));
    if (hipGetLastError() != hipSuccess) return -5;
  }
  return 0;
}

template <bool SCALED, int METRIC>
int launch_all(const Layout &L, const Arena &ar, int *out, hipStream_t s) {
  int rc = launch_kind<K16, SCALED, METRIC>(L, ar, out, s);
  if (rc == 0) rc = launch_kind<K32, SCALED, METRIC>(L, ar, out, s);
  if (rc == 0) rc = launch_kind<K64, SCALED, METRIC>(L, ar, out, s);
  if (rc == 0) rc = launch_kind<K128, SCALED, METRIC>(L, ar, out, s);
  if (rc == 0) rc = launch_kind<K256, SCALED, METRIC>(L, ar, out, s);
  return rc;
}

// The matcher kernels of one request: its metric's, for its code scaling.
int launch_metric(const Layout &L, const Arena &ar, int metric, int *out, hipStream_t s) {
  if (metric == METRIC_LEVENSHTEIN)
    return L.scaled ? launch_all<true, METRIC_LEVENSHTEIN>(L, ar, out, s)
                    : launch_all<false, METRIC_LEVENSHTEIN>(L, ar, out, s);
  return L.scaled ? launch_all<true, METRIC_INDEL2>(L, ar, out, s) : launch_all<false, METRIC_INDEL2>(L, ar, out, s);
}

// The merge of a top-k request: one launch per class, one wave per query slot
// of the class's tiles, whatever slabs they were launched in.
int launch_merge(const Layout &L, const Arena &ar, hipStream_t s) {
  for (int kind = 0; kind < NKINDS; kind++) {
    if (L.kindCount[kind] == 0) continue;
    const int slots = L.kindCount[kind] * kKindQueries[kind];
    hipLaunchKernelGGL(ed_topk_merge_kernel, dim3((slots + THREADS / 64 - 1) / (THREADS / 64)), dim3(THREADS), 0, s,
                       reinterpret_cast<const u64 *>(ar.out) + L.partOff[kind],
                       dev_at<const int>(ar, L.oTileQ) + (size_t)L.kindStart[kind] * kTileSlots, kKindQueries[kind],
                       slots, L.partCount[kind], L.k, dev_at<u64>(ar, L.oBest));
    if (hipGetLastError() != hipSuccess) return -5;
  }
  return 0;
}

// The fill kernel of the normalising modes: one lane per panel slot.
int launch_fill(const Layout &L, const Arena &ar, hipStream_t s) {
  hipLaunchKernelGGL(ed_fill_panels_kernel, dim3(L.nPanels * (SLOTS / THREADS)), dim3(THREADS), 0, s,
                     dev_at<const uint4>(ar, L.oRaw), dev_at<const int64_t>(ar, L.oOffA),
                     dev_at<const int>(ar, L.oPerm), dev_at<const int64_t>(ar, L.oPanelOff),
                     dev_at<const int>(ar, L.oPanelBlocks), dev_at<const uint32_t>(ar, L.oByteMap),
                     dev_at<uint4>(ar, L.oPanels), dev_at<int>(ar, L.oLenSorted));
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// ev[0] .. ev[3] bracket H2D, the kernels and D2H; with a device fill ev[4]
// lies between the fill kernel and the matcher kernels.
void record_times(Arena &ar, double prep, bool deviceFill) {
  float a = 0, b = 0, c = 0, f = 0;
  (void)hipEventElapsedTime(&a, ar.ev[0], ar.ev[1]);
  if (deviceFill) (void)hipEventElapsedTime(&f, ar.ev[1], ar.ev[4]);
  (void)hipEventElapsedTime(&b, ar.ev[deviceFill ? 4 : 1], ar.ev[2]);
  (void)hipEventElapsedTime(&c, ar.ev[2], ar.ev[3]);
  ar.last[0] = prep;
  ar.last[1] = a;
  ar.last[2] = b;
  ar.last[3] = c;
  ar.last[4] = f;
  if (getenv("M2K_ED_PROFILE"))
    fprintf(stderr, "[m2k_ed] prep %.3f ms  h2d %.3f ms  fill %.3f ms  kernel %.3f ms  d2h %.3f ms\n", prep, a, f, b,
            c);
}

// One request: the distance matrix into outT when it is set, the closest
// option per query into bestIdx / bestDist otherwise; with `groupOf` (the
// group of every option, nGroups of them) the closest option per query and
// group, bestIdx / bestDist query-major [nB * nGroups], -1 / -1 for a group
// without options; with `topk` the k closest options per query, bestIdx /
// bestDist query-major [nB * k] in (distance, index) order, -1 / -1 behind the
// last option.  Its kernels leave one list per wave in a device-only partial
// buffer, which ed_topk_merge_kernel folds into `best`; both count as kernel
// time.
// `mode` is MODE_NONE (the strings are matched as they are, the host fills the
// panels) or a normalising mode (raw strings in, the device fills the panels
// under the mode's byte map; the query limit then applies to the normalised
// query).
// `metric` is METRIC_INDEL2 (ins = del = 1, sub = 2: the LCS kernels) or
// METRIC_LEVENSHTEIN (ins = del = sub = 1: the Myers kernels); everything
// before and after the matcher kernels is the same for both.
//   step                                 returns
//   unknown mode                         -9
//   unknown metric                       -10
//   groups: nGroups < 1, a group id
//   outside [0, nGroups)                 -11 (before anything is allocated)
//   top-k: k outside [1, K_MAX]          -12 (before anything is allocated)
//   no device                            -1
//   nothing to compute                   0 (closest without options: -1 / -1 per query)
//   prepare                              -2 query too long, -8 no free byte code, -4 arena
//   matrix: device output buffer,
//   top-k: device partial buffer         -4
//   H2D copy                             -7, at once (no sync)
//   closest: memset of `best` (top-k:
//   and of the partial buffer)           -4, at once (no sync)
//   a kernel launch (the fill included)  -5  } later launches and the D2H copy are
//   D2H copy                             -7  } skipped, the stream is synchronised
//   stream synchronise                   -6 (when nothing failed before)
// Timings are recorded on success only.
// `names` is the names route (ed_closest_names_kernel): opts / nA are then the
// names (the panel side, any length), qs / nB the options (the tile side, the
// 256-byte limit and -2 are theirs), groupOf the options' groups (nullptr: one
// group), and bestIdx / bestDist name-major [nA * nGroups], indices into the
// options; without options every entry is -1 / -1.
int run(const uint8_t *opts, const int64_t *offA, int nA, const uint8_t *qs, const int64_t *offB, int nB,
        int32_t *outT, int32_t *bestIdx, int32_t *bestDist, int mode = MODE_NONE, int metric = METRIC_INDEL2,
        const int32_t *groupOf = nullptr, int nGroups = 0, bool topk = false, int k = 0, bool names = false) {
  if (mode != MODE_NONE && mode != MODE_ALNUM_LOWER) return -9;
  if (metric != METRIC_INDEL2 && metric != METRIC_LEVENSHTEIN) return -10;
  if (groupOf) {
    if (nGroups < 1) return -11;
    for (int i = 0; i < (names ? nB : nA); i++)
      if (groupOf[i] < 0 || groupOf[i] >= nGroups) return -11;
  }
  if (topk && (k < 1 || k > K_MAX)) return -12;
  if (names && !groupOf) nGroups = 1;
  // who asks and what they choose among: the queries and the options, on the
  // names route the names (the panel side there) and the options (the tile side)
  const int nAsk = names ? nA : nB, nPick = names ? nB : nA;
  const size_t nBest = (size_t)std::max(nAsk, 0) * (size_t)(topk ? k : groupOf || names ? nGroups : 1);
  const bool deviceFill = mode != MODE_NONE;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return -1;
  if (nAsk <= 0 || (outT && nPick <= 0)) return 0;
  if (nPick <= 0) {
    for (size_t j = 0; j < nBest; j++) bestIdx[j] = -1, bestDist[j] = -1;
    return 0;
  }
  Arena &ar = arena();
  std::lock_guard<std::mutex> lock(ar.mu);
  const double t0 = now_ms();
  Layout L;
  L.k = topk ? k : 0;
  int rc = deviceFill ? prepare_norm(opts, offA, nA, groupOf, nGroups, qs, offB, nB, mode, ar, L, names)
                      : prepare(opts, offA, nA, groupOf, nGroups, qs, offB, nB, ar, L, names);
  if (rc) return rc;
  if (outT && (rc = ar.ensure_out(sizeof(int) * (size_t)nA * nB))) return rc;
  if (topk && (rc = ar.ensure_out(sizeof(u64) * L.partKeys))) return rc;
  const double prep = now_ms() - t0;
  u64 *best = dev_at<u64>(ar, L.oBest), *hBest = reinterpret_cast<u64 *>(ar.host + L.oBest);
  hipStream_t s = ar.stream;
  (void)hipEventRecord(ar.ev[0], s);
  if (hipMemcpyAsync(ar.dev, ar.host, L.h2dBytes, hipMemcpyHostToDevice, s) != hipSuccess) return -7;
  if (!outT && hipMemsetAsync(best, 0xff, sizeof(u64) * nBest, s) != hipSuccess) return -4;
  if (topk && hipMemsetAsync(ar.out, 0xff, sizeof(u64) * L.partKeys, s) != hipSuccess) return -4;
  (void)hipEventRecord(ar.ev[1], s);
  int *out = outT ? ar.out : nullptr;
  if (deviceFill) {
    rc = launch_fill(L, ar, s);
    (void)hipEventRecord(ar.ev[4], s);
  }
  if (rc == 0) rc = launch_metric(L, ar, metric, out, s);
  if (rc == 0 && topk) rc = launch_merge(L, ar, s);
  (void)hipEventRecord(ar.ev[2], s);
  if (rc == 0) {
    const hipError_t e = outT ? hipMemcpyAsync(outT, out, sizeof(int) * (size_t)nA * nB, hipMemcpyDeviceToHost, s)
                              : hipMemcpyAsync(hBest, best, sizeof(u64) * nBest, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) rc = -7;
  }
  (void)hipEventRecord(ar.ev[3], s);
  if (hipStreamSynchronize(s) != hipSuccess && rc == 0) rc = -6;
  if (rc) return rc;
  if (!outT)  // (a key still ~0, a group without options, unpacks to -1 / -1)
    for (size_t j = 0; j < nBest; j++) {
      bestIdx[j] = (int32_t)(hBest[j] & 0xffffffffULL);
      bestDist[j] = (int32_t)(hBest[j] >> 32);
    }
  record_times(ar, prep, deviceFill);
  return 0;
}

}  // namespace

extern "C" {

// Full distance matrix, query-major: outT[j * nA + i] = dist(opts[i], queries[j]).
// Strings are packed back to back with (n+1) int64 offsets.  Queries must be <= 256 bytes
// (-2 otherwise).  Returns 0 on success, negative on error.
int m2k_ed_matrix(const uint8_t *opts, const int64_t *offA, int nA, const uint8_t *qs, const int64_t *offB, int nB,
                  int32_t *outT) {
  return run(opts, offA, nA, qs, offB, nB, outT, nullptr, nullptr);
}

// Closest option per query: bestIdx[j] = first i minimising dist(opts[i], queries[j]),
// bestDist[j] = that distance (-1/-1 when there are no options).
int m2k_ed_closest(const uint8_t *opts, const int64_t *offA, int nA, const uint8_t *qs, const int64_t *offB, int nB,
                   int32_t *bestIdx, int32_t *bestDist) {
  return run(opts, offA, nA, qs, offB, nB, nullptr, bestIdx, bestDist);
}

// The same two on raw strings under a normalising mode (1 = ALNUM_LOWER: keep
// 0-9 a-z A-Z, fold A-Z to a-z, drop every other byte): the distances are those
// of the normalised strings.  The queries must be <= 256 bytes after
// normalisation (-2 otherwise); an unknown mode returns -9.
int m2k_ed_matrix_norm(const uint8_t *opts, const int64_t *offA, int nA, const uint8_t *qs, const int64_t *offB,
                       int nB, int mode, int32_t *outT) {
  return run(opts, offA, nA, qs, offB, nB, outT, nullptr, nullptr, mode);
}

int m2k_ed_closest_norm(const uint8_t *opts, const int64_t *offA, int nA, const uint8_t *qs, const int64_t *offB,
                        int nB, int mode, int32_t *bestIdx, int32_t *bestDist) {
  return run(opts, offA, nA, qs, offB, nB, nullptr, bestIdx, bestDist, mode);
}

// The same two under a metric (0 = ins 1, del 1, sub 2 as above; 1 = unit-cost
// Levenshtein) and a mode (0 = the strings as they are, 1 = ALNUM_LOWER), in any
// combination; an unknown metric returns -10.
int m2k_ed_matrix_metric(const uint8_t *opts, const int64_t *offA, int nA, const uint8_t *qs, const int64_t *offB,
                         int nB, int mode, int metric, int32_t *outT) {
  return run(opts, offA, nA, qs, offB, nB, outT, nullptr, nullptr, mode, metric);
}

int m2k_ed_closest_metric(const uint8_t *opts, const int64_t *offA, int nA, const uint8_t *qs, const int64_t *offB,
                          int nB, int mode, int metric, int32_t *bestIdx, int32_t *bestDist) {
  return run(opts, offA, nA, qs, offB, nB, nullptr, bestIdx, bestDist, mode, metric);
}

// Closest option per query and group: groupOf[i] in [0, nGroups) is the group
// of option i.  bestIdx[j * nGroups + g] = first i of group g minimising
// dist(opts[i], queries[j]), bestDist the distance, -1 / -1 for a group
// without options.  Mode and metric as above; a group id out of range or
// nGroups < 1 returns -11.  With nGroups == 1 the answer is m2k_ed_closest_metric's.
int m2k_ed_closest_grouped(const uint8_t *opts, const int64_t *offA, int nA, const int32_t *groupOf, int nGroups,
                           const uint8_t *qs, const int64_t *offB, int nB, int mode, int metric, int32_t *bestIdx,
                           int32_t *bestDist) {
  static const int32_t none = 0;  // no options and no group array: still a grouped request
  if (!groupOf && nA > 0) return -11;
  return run(opts, offA, nA, qs, offB, nB, nullptr, bestIdx, bestDist, mode, metric, groupOf ? groupOf : &none,
             nGroups);
}

// The k closest options per query, k in [1, 64] (-12 otherwise): bestIdx[j * k + r]
// = the option of rank r in (distance, index) order, so r = 0 is m2k_ed_closest_metric's
// answer, bestDist its distance, -1 / -1 from rank nA on.  Mode and metric as above.
int m2k_ed_closest_k(const uint8_t *opts, const int64_t *offA, int nA, const uint8_t *qs, const int64_t *offB, int nB,
                     int k, int mode, int metric, int32_t *bestIdx, int32_t *bestDist) {
  return run(opts, offA, nA, qs, offB, nB, nullptr, bestIdx, bestDist, mode, metric, nullptr, 0, true, k);
}

// Many names against a few options: m2k_ed_closest_grouped's answer with the
// sides' roles swapped on the device (the names in the lanes, the options'
// tables in LDS), for nB much larger than nA.  bestIdx / bestDist are laid out
// exactly as there: [nB * nGroups], name-major, indices into the flat options,
// -1 / -1 for a group without options; groupOf == nullptr is one group (nGroups
// is then ignored).  The 256-byte limit is on the options here (-2; in a
// normalising mode after normalisation) and the names may be of any length.
// Other codes as m2k_ed_closest_grouped.
int m2k_ed_closest_names(const uint8_t *opts, const int64_t *offA, int nA, const int32_t *groupOf, int nGroups,
                         const uint8_t *names, const int64_t *offB, int nB, int mode, int metric, int32_t *bestIdx,
                         int32_t *bestDist) {
  return run(names, offB, nB, opts, offA, nA, nullptr, bestIdx, bestDist, mode, metric, groupOf, nGroups, false, 0,
             true);
}

// prep / H2D / kernel / D2H milliseconds of the last successful call
void m2k_ed_last_timings(double *out4) {
  Arena &ar = arena();
  std::lock_guard<std::mutex> lock(ar.mu);
  for (int i = 0; i < 4; i++) out4[i] = ar.last[i];
}

// Milliseconds of the fill kernel in the last successful call (0 when the host
// filled the panels); the kernel time above does not include it.
double m2k_ed_last_fill_ms() {
  Arena &ar = arena();
  std::lock_guard<std::mutex> lock(ar.mu);
  return ar.last[4];
}

int m2k_gpu_device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char *m2k_gpu_arch() {
  static char name[256];
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, 0) != hipSuccess) return "";
  strncpy(name, p.gcnArchName, sizeof(name) - 1);
  return name;
}
}
