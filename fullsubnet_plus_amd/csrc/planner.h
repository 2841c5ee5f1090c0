// planner.h - the sub-band planner of libfsnp_hip.so: which kernel runs which sequences.  Host-only code (planner.cpp), driven by a
// cost table; CPU-tested through fsnp_debug_plan_rows / fsnp_debug_plan_rows2 (tests/test_host.py).
#pragma once
#include <vector>

namespace fsnp {

// per-step cost table of the sub-band planner (see default_costs / calibrate_costs); flat layout: costs_to_array (fsnp.h: FSNP_NUM_COSTS)
struct CostTable {
    double ksplit[4][2];       // K-split kernel at 8 / 16 / 32 / 64 units per workgroup x {<= 1, 2} workgroups per CU, launch FULL
    double ksplit1[4];         // the same with ONE row tile (the exchange traffic, hence a step, grows with the tiles in flight)
    double coopn[2][2];        // three-way split, 1 / 2 row tiles per group x {<= 1, 2} workgroups per CU
    double rowtile, rowtile_ex;   // one round of the one-tile-per-CU kernel; relative extra per VALU row
    double rowtile16;             // one round of the half-tile (16-row) kernel (lstm16.hip)
    double hp[2];                 // half-tile ping-pong (lstm_hp.hip, 16 units): ONE row tile, a FULL launch (num_cus / (H / 16) tiles)
    double coopw[3][2];           // wave-owned column split (lstm_coopw.hip) at 32 / 64 / 96 units per workgroup: ONE row tile, a FULL launch
    int calibrated;
};

// ---- plan of the sub-band recurrent model: which kernel runs which sequences.
// The row-tile kernel (lstm.hip) needs >= 256 tiles to fill the chip and costs ~208 us per step however few tiles it
// gets; the column-split kernels pay one inter-workgroup barrier per step instead:
//   <= 42 row tiles  : lstm_coop.hip  (K split, 8..64 hidden units per workgroup, row_tiles * H/units <= CUs)
//   43..170 row tiles: lstm_coopn.hip (3 workgroups x 128 units share 1-2 row tiles)
// A problem is cut into CHUNKS of consecutive sequences that run back to back: e.g. B = 40 (10280 sequences) = one full
// round of the row-tile kernel (8192) + 66 tiles on lstm_coopn.hip instead of two rounds; GRU (column-split only) =
// chunks of <= 170 tiles.  Every chunk owns a slice of the row descriptors / per-row norm tables (slot0) and, if it is
// column-split, of the exchange images and barrier counters (coop_tile0).
// the kind of a chunk = which kernel runs it (the numbers are those fsnp_debug_plan_rows* report)
enum class SbKind : int {
    RowTile = 0,               // one 32-row tile per CU (lstm.hip / lstm_gru.hip; VALU rows: 32 + ex slots per tile)
    KSplit = 1,                // column split: K split, 8 .. 64 hidden units per workgroup (lstm_coop.hip)
    ThreeWay = 2,              // column split: 3 workgroups x 128 units share 1 - 2 row tiles (lstm_coopn.hip)
    HalfTile = 4,              // one 16-row tile per CU (lstm16.hip; rps = 16)
    Generic = 7,               // runtime-sized kernel, workgroups of rpg sequences (lstm_generic.hip)
    HalfTilePingPong = 8,      // column split: H / 16 workgroups per row tile (lstm_hpw.hip, FSNP_HP_WAVE=0: lstm_hp.hip)
    WaveOwned = 9,             // column split: 32 / 64 / 96 units per workgroup, one per CU (lstm_coopw.hip)
};
bool is_column_split(SbKind k);     // the kinds whose workgroups exchange state each step (exchange images, barrier counters)

struct SbChunk {
    SbKind kind;
    int row0, nrows;           // sequences [row0, row0 + nrows)
    int num_tiles, ex, rps;    // tiles, VALU rows per tile, slots per tile (32 + ex)
    int units, groups, rpg;    // column-split parameters
    int slot0, coop_tile0;
};
inline SbChunk row_tile_chunk(int row0, int nrows, int tiles, int ex = 0, int rps = 32) { return {SbKind::RowTile, row0, nrows, tiles, ex, rps, 0, 0, 0, 0, 0}; }
inline SbChunk half_tile_chunk(int row0, int nrows, int tiles) { return {SbKind::HalfTile, row0, nrows, tiles, 0, 16, 0, 0, 0, 0, 0}; }
inline SbChunk generic_chunk(int row0, int nrows, int rpg) { return {SbKind::Generic, row0, nrows, (nrows + rpg - 1) / rpg, 0, rpg, 0, 0, rpg, 0, 0}; }
// a column-split launch: `units` hidden units per workgroup (ThreeWay: 0, and cdiv(tiles, rpg) groups of rpg row tiles; others: rpg = 0)
inline SbChunk column_chunk(SbKind kind, int row0, int nrows, int tiles, int units, int rpg) {
    return {kind, row0, nrows, tiles, 0, 32, units, kind == SbKind::ThreeWay ? (tiles + rpg - 1) / rpg : 0, rpg, 0, 0};
}
struct SbPlan {
    std::vector<SbChunk> chunks;
    int total_slots = 0, coop_tiles = 0;
};

struct PlannerOptions {        // what a handle decides about its plans besides its sizes (fsnp_handle::planner)
    bool rowtile_ok = true, lstm16_ok = false, hp_ok = false, coopw_ok = false;   // kernels that exist for the sub-band model
    int lstm_coop = 1, coop_hp = 0, coop_w = 0, coop_occ = 1;                       // what the switches allow of them
    int occ_ksplit[4] = {1, 1, 1, 1}, occ_coopn[2] = {1, 1};                        // workgroups per CU each instantiation fits
    double composite_gain = 0.97;
    CostTable cost{};
};
// FSNP_LSTM16, FSNP_LSTM_COOP, FSNP_COOP_HP, FSNP_COOP_W, FSNP_COOP_OCC as fsnp_create reads them (defaults: unset)
struct PlannerSwitches { bool lstm16 = true; int lstm_coop = 1, coop_hp = 1, coop_w = 1, coop_occ = 2; };
// which sub-band kernels exist for the model (seq_model: FSNP_SEQ_*; generic_sb: it runs on lstm_generic.hip) and what the switches
// allow of them; the cost table and the occupancies keep their defaults
PlannerOptions planner_options(int seq_model, int sb_hidden, int nin, bool generic_sb, const PlannerSwitches& sw);

// what the planner needs to know of a handle (fsnp_abi.hip: pctx)
struct PlannerCtx : PlannerOptions {
    int H = 0, NIN = 0, num_cus = 256, num_cus_real = 256;
    bool gru = false, sb_tcn = false, generic_sb = false; int ih_bf16 = 0;
    bool half_tiles_without_coop = false;   // lstm_coop == 0 plans may still use the (exchange-free) half-tile kernel: fsnp_set_verify's re-run
};

CostTable default_costs();
// the flat table of fsnp_get_costs / fsnp_debug_set_costs (include/fsnp.h: FSNP_NUM_COSTS values)
constexpr int kNumCosts = 27;
void costs_to_array(const CostTable& t, double* out);
void costs_from_array(CostTable& t, const double* in);
// the table a handle starts from: the built-in one scaled to the handle's cell and hidden size (measured at LSTM, H = 384)
CostTable initial_costs(int sb_hidden, bool gru, bool sb_tcn);
// S workgroups per row tile and the T tiles (ThreeWay: groups) a launch of chunk c decodes: S * T workgroups (S = 1 unless column split)
struct SbSplit { int S, T; };
SbSplit chunk_split(const PlannerCtx& h, const SbChunk& c);
int chunk_workgroups(const PlannerCtx& h, const SbChunk& c);
double est_step_us(const PlannerCtx& h, const SbChunk& c);
SbPlan plan_sb(const PlannerCtx& h, int num_rows);       // empty plan = "this device cannot run the model"
// the kernel code fsnp_describe_plan reports for a chunk (include/fsnp.h); hpw: HalfTilePingPong launches run on lstm_hpw.hip
int describe_code(SbKind k, bool sb_tcn, bool hpw);
// pipelined serving loop (fsnp_set_pipeline): the first chunk that goes to the side stream (== chunks.size(): none; 0: the whole plan)
int plan_first_deferred(const PlannerCtx& h, const SbPlan& plan, bool defer_small);

// ---- may two column-split launches of one handle run side by side?  All the workgroups of each must be co-resident, and the
// dispatcher deals workgroup id i to XCD i % 8 whatever room that XCD has: what has to fit is counted per XCD, not per chip.
constexpr int kNumXcds = 8;
struct CoopFootprint {
    int per_xcd[kNumXcds];     // workgroups dealt to each XCD (those of an XCD-local launch that find no row tile exit at once: counted too)
    int own_cu;                // 1: each workgroup claims a whole CU (LstmArgs::coop_own_cu), nothing else runs beside it there
    int per_cu;                // workgroups of this kernel one CU holds at once (hipOccupancyMaxActiveBlocksPerMultiprocessor); <= 0: unknown
};
// a launch of `wgs` workgroups dealt round robin (coop_xcd = 0)
CoopFootprint coop_footprint_round_robin(int wgs, bool own_cu, int per_cu);
// the CUs per XCD launch_sb_lstm passes as LstmArgs::coop_xcd for chunk c (XCD-local placement, lstm_common.h), 0 = round robin
int chunk_coop_xcd(const PlannerCtx& h, const SbChunk& c);
// where chunk c's workgroups go (the placement launch_sb_lstm uses)
CoopFootprint chunk_footprint(const PlannerCtx& h, const SbChunk& c, bool own_cu, int per_cu);
// Side by side only if one of the two can ALWAYS become fully resident, whatever the other holds: on every XCD the CUs the other may
// occupy (at most one per workgroup dealt there) plus the CUs this one needs at its own occupancy (one per workgroup if it owns its
// CUs, else cdiv(workgroups there, per_cu)) fit in the XCD.  That one then runs to its end and frees its CUs for the other.
// Unknown occupancy or CU count: false (chain them).
bool coop_side_by_side(const CoopFootprint& a, const CoopFootprint& b, int cus_per_xcd);
// two launches that may be in flight together, as one blocker: one whole CU per workgroup (for a further side-by-side check)
CoopFootprint coop_footprint_sum(const CoopFootprint& a, const CoopFootprint& b);

}  // namespace fsnp
