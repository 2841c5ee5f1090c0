"""The cases of tests/test_gpu_subband.py, kept apart from it so that the CPU suite can check each case's plan against the host-only
planner (fsnp_debug_plan_rows2) where no GPU is: a case names the hooks that force its kernel path and states the plan they give.

A plan is a list of launches P(kind, rows, tiles, ex, par, rpg) in the planner's own terms (csrc/planner.h SbKind: 0 one 32-row tile per
CU - ex VALU rows per tile; 1 K split at `par` units per workgroup; 2 three-way split, `par` groups of `rpg` row tiles; 4 one 16-row
tile per CU; 8 half-tile ping-pong; 9 wave-owned column split at `par` units).  Cases whose model the host planner does not describe
(another hidden size, more than 64 input features, the TCN) name the kernels they expect instead (`kernels`).
"""
from oracle.ref_loader import DEFAULT_MODEL_ARGS, FULLSUBNET_MODEL_ARGS
from oracle.weights import make_state_dict, make_state_dict_fullsubnet
from tests._util import edge_lengths

CUMULATIVE = ("cumulative_laplace_norm", "cumulative_layer_norm")
NORMS = ("offline_laplace_norm", "offline_gaussian_norm") + CUMULATIVE


# ------------------------------------------------------------------------------------------------ cost tables (fsnp_get_costs layout)
def ksplit_only_costs(units):
    """K split (csrc/lstm_coop.hip) at `units` per workgroup cheap - a full launch and one tile - everything else priced out (19 values:
    the half-tile ping-pong kernel and the wave-owned split are not named at all)."""
    i = (8, 16, 32, 64).index(units)
    full, one = [900.0] * 8, [900.0] * 4
    full[2 * i], one[i] = 5.0, 5.0
    return full + [900.0] * 4 + [900.0, 0.11] + one + [900.0]


def coopn_only_costs(rpg):
    """Three-way split (csrc/lstm_coopn.hip) with `rpg` row tiles per group cheap."""
    c = [900.0] * 4
    c[2 * (rpg - 1)] = 5.0
    return [900.0] * 8 + c + [900.0, 0.11] + [900.0] * 4 + [900.0]


def hp_only_costs():
    """Every column-split launch is the half-tile ping-pong kernel (tests/test_gpu_parity.py _hp_only_costs)."""
    return [900.0] * 12 + [900.0, 0.11] + [900.0] * 4 + [900.0] + [5.0, 5.0]


def coopw_only_costs(units):
    """Every column-split launch is the wave-owned split at `units` (tests/test_gpu_parity.py _coopw_only_costs)."""
    w = [5.0 if 32 * (i + 1) == units else 900.0 for i in range(2)]
    w96 = [5.0, 5.0] if units == 96 else [900.0, 900.0]
    return [900.0] * 12 + [900.0, 0.11] + [900.0] * 4 + [900.0] + [900.0, 900.0] + w + w + w96


def half_tile_only_costs():
    """The 16-row tile kernel (csrc/lstm16.hip) is the cheapest shape at any size (tests/test_gpu_parity.py test_half_tile_kernel)."""
    return [900.0] * 8 + [900.0] * 4 + [900.0, 0.11] + [900.0] * 4 + [10.0]


# the built-in table (csrc/planner.cpp default_costs), written out so that a case pins its plan whatever a handle has calibrated
BUILT_IN = [8.4, 25.2, 14.2, 42.6, 24.8, 74.4, 49.2, 147.6, 84.0, 184.8, 154.0, 338.8, 206.0, 0.11, 8.0, 13.3, 22.7, 45.6, 103.0,
            10.4, 11.0, 22.3, 38.5, 21.0, 37.0, 56.5, 52.5]
TABLES = {"built_in": BUILT_IN, "built_in_19": BUILT_IN[:19], "hp": hp_only_costs(), "half_tile": half_tile_only_costs(),
          **{f"ks{u}": ksplit_only_costs(u) for u in (8, 16, 32, 64)}, **{f"cw{u}": coopw_only_costs(u) for u in (32, 64, 96)},
          **{f"cn{r}": coopn_only_costs(r) for r in (1, 2)}}


def P(kind, rows, tiles, ex=0, par=0, rpg=0):
    return (kind, rows, tiles, ex, par, rpg)


# ------------------------------------------------------------------------------------------------ the cases
CASES = {}


def case(name, plan=None, **kw):
    """model "plus" / "fsn"; over: model arguments that differ from the default ones; mode "full" / "parity"; lengths: a ragged pool;
    coop / cus / waves / costs: debug_set_lstm_coop, debug_set_num_cus, debug_set_lstm_waves, debug_set_costs (a TABLES name);
    plan: the launches (above), checked on the CPU with the host planner unless host=False; kernels: kernel-name prefixes expected
    instead, where there is no plan; pp: which file runs kind 8 ("hpw" / "hp"); same_as / differs_from: another case of the same model
    and input whose mask must be bit-equal / must not be."""
    c = dict(name=name, model="plus", over={}, profile="harsh", B=2, T=22, F=257, mode="full", lengths=None, coop=1, cus=None, waves=None,
             costs="built_in", plan=plan, host=plan is not None, kernels=None, pp="hpw", same_as=None, differs_from=None, seed=0)
    assert set(kw) <= set(c), set(kw) - set(c)
    c.update(kw)
    assert name not in CASES and (c["plan"] is None) != (c["kernels"] is None)
    assert c["T"] + model_args(c)["look_ahead"] <= 48 or name.startswith("cum_chunks_"), name
    CASES[name] = c


def model_args(c):
    base = FULLSUBNET_MODEL_ARGS if c["model"] == "fsn" else DEFAULT_MODEL_ARGS
    return dict(base, num_freqs=c["F"], **c["over"])


def plus_state_dict(seed, profile, args):
    return make_state_dict(seed, profile, num_freqs=args["num_freqs"], sb_hidden=args["sb_model_hidden_size"],
                           sb_num_neighbors=args["sb_num_neighbors"], fb_num_neighbors=args["fb_num_neighbors"],
                           kersize=tuple(args.get("kersize", (3, 5, 10))), output_size=args.get("output_size", 2),
                           attention=args.get("channel_attention_model", "TSSE"), sequence_model=args["sequence_model"])


def state_dict(c):
    args = model_args(c)
    if c["model"] == "fsn":
        return make_state_dict_fullsubnet(21, c["profile"], num_freqs=args["num_freqs"], fb_num_neighbors=args["fb_num_neighbors"])
    return plus_state_dict(21, c["profile"], args)


def rows_of(c):
    """Sub-band sequences of the case's forward: every bin of every utterance, or what drop_band keeps (feature.py:254-285)."""
    g = model_args(c)["num_groups_in_drop_band"]
    return c["B"] * (c["F"] // g if c["mode"] == "parity" and g > 1 else c["F"])


# 1. one 32-row tile per CU (csrc/lstm.hip): VALU rows 0 / 1 / 2 / 4 by bin count x batch x pretend CUs, several rounds, 4 and 12 waves,
#    ragged last tiles (257 = 8 x 32 + 1 = 7 x 33 + 26, 514 = 16 x 32 + 2 = 14 x 36 + 10, 644 = 18 x 34 + 32, 322 = 8 x 36 + 34)
case("rt_ex0_two_rounds", [P(0, 257, 14)], B=1, coop=0, cus=7, profile="default")
case("rt_ex1_waves12", [P(0, 257, 8, 1)], B=1, coop=0, cus=8, waves=12)
case("rt_ex1_waves4", [P(0, 257, 8, 1)], B=1, coop=0, cus=8, waves=4)
case("rt_ex2_f161_b4", [P(0, 644, 19, 2)], B=4, F=161, T=10, coop=0, cus=19)
case("rt_ex4_three_rounds", [P(0, 514, 15, 4)], coop=0, cus=5)
case("rt_ex4_f161", [P(0, 322, 9, 4)], F=161, coop=0, cus=9, profile="default", waves=4)
case("rt_b2", [P(0, 514, 17)], coop=0)
case("rt_b1", [P(0, 257, 9)], B=1, coop=0)
# 2. one 16-row tile per CU (csrc/lstm16.hip), forced through the cost table: last tiles of one and of two rows
case("half_tile_b1", [P(4, 257, 17)], B=1, costs="half_tile", differs_from="rt_b1")
case("half_tile_f161_b2", [P(4, 322, 21)], F=161, costs="half_tile", profile="default")
# 3. K split (csrc/lstm_coop.hip) at 8 / 16 / 32 / 64 units: several tiles, and ONE tile (the second launch of 161 = 160 + 1 rows at 8
#    units, where a launch holds five tiles); the serial schedule (mode 2) must give the skewed one's bits
case("ks8_f161_b1", [P(1, 160, 5, par=8), P(1, 1, 1, par=8)], B=1, F=161, costs="ks8")
case("ks16_b1", [P(1, 257, 9, par=16)], B=1, costs="ks16", differs_from="rt_b1")
case("ks16_b1_serial", [P(1, 257, 9, par=16)], B=1, costs="ks16", coop=2, same_as="ks16_b1")
case("ks32_b2", [P(1, 514, 17, par=32)], costs="ks32", differs_from="rt_b2")
case("ks64_b2", [P(1, 514, 17, par=64)], costs="ks64", differs_from="rt_b2")
case("ks64_b2_serial", [P(1, 514, 17, par=64)], costs="ks64", coop=2, same_as="ks64_b2")
# 4. three-way split (csrc/lstm_coopn.hip): one and two row tiles per group (25 tiles: the last group of two holds one), forced; and
#    where the planner takes it by itself without the round-5 kernels (B = 8)
case("cn1_b3", [P(2, 771, 25, par=25, rpg=1)], B=3, T=8, costs="cn1")
case("cn2_b3", [P(2, 771, 25, par=13, rpg=2)], B=3, T=8, costs="cn2")
case("cn2_b6", [P(2, 1542, 49, par=25, rpg=2)], B=6, T=8, costs="cn2", profile="default")
case("cn1_b8_planned", [P(2, 2056, 65, par=65, rpg=1)], B=8, T=8, costs="built_in_19", profile="default")
# 5. half-tile ping-pong: lstm_hpw.hip (34 inputs) and lstm_hp.hip (46 inputs: fb_num_neighbors 2), B = 1 (the last tile holds one row) and 2
case("hpw_b1", [P(8, 257, 9)], B=1, coop=4, costs="hp", differs_from="rt_b1")
case("hpw_b2", [P(8, 320, 10), P(8, 194, 7)], coop=4, costs="hp", differs_from="rt_b2")
case("hp_fbn2_b1", [P(8, 257, 9)], B=1, coop=4, costs="hp", over=dict(fb_num_neighbors=2), pp="hp")
case("hp_fbn2_b2", [P(8, 320, 10), P(8, 194, 7)], coop=4, costs="hp", over=dict(fb_num_neighbors=2), pp="hp", profile="default")
# 6. wave-owned column split (csrc/lstm_coopw.hip) at 32 / 64 / 96 units; one launch plus a remainder on the K split
case("cw32_b1", [P(9, 257, 9, par=32)], B=1, costs="cw32", differs_from="rt_b1")
case("cw64_b2", [P(9, 514, 17, par=64)], costs="cw64", differs_from="rt_b2")
case("cw96_b2", [P(9, 514, 17, par=96)], costs="cw96", differs_from="rt_b2")
case("cw32_plus_ks8_b3", [P(9, 672, 21, par=32), P(1, 99, 4, par=8)], B=3, T=10)
# 7. fb_num_neighbors 2 and 3 (46 / 52 inputs: the K = 64 instantiations; refl_wfb at both band edges), another sb_num_neighbors
case("fbn2_rt", [P(0, 257, 9)], B=1, coop=0, over=dict(fb_num_neighbors=2))
case("fbn2_cw32", [P(9, 257, 9, par=32)], B=1, costs="cw32", over=dict(fb_num_neighbors=2), differs_from="fbn2_rt")
case("fbn3_rt", [P(0, 257, 9)], B=1, coop=0, over=dict(fb_num_neighbors=3), profile="default")
case("fbn3_hp", [P(8, 257, 9)], B=1, coop=4, costs="hp", over=dict(fb_num_neighbors=3), pp="hp", profile="default")
case("sbn10_cw32", [P(9, 514, 17, par=32)], over=dict(sb_num_neighbors=10))
# 8. other sub-band models
case("generic_hidden320", kernels=("lstm2_generic_kernel",), B=1, T=10, over=dict(sb_model_hidden_size=320))
case("generic_fbn6", kernels=("lstm2_generic_kernel",), B=1, T=10, over=dict(fb_num_neighbors=6))
case("hidden256_rt", [P(0, 257, 9)], B=1, coop=0, over=dict(sb_model_hidden_size=256), host=False)
case("hidden256_column_split", kernels=("lstm2_coop",), B=1, over=dict(sb_model_hidden_size=256), costs=None)
case("hidden512_column_split", kernels=("lstm2_coop",), B=1, over=dict(sb_model_hidden_size=512), costs=None)
case("hidden256_fbn2_rt", [P(0, 257, 9)], B=1, coop=0, over=dict(sb_model_hidden_size=256, fb_num_neighbors=2), host=False)   # (H = 256 at K = 64)
case("gru_rt", [P(0, 257, 9)], B=1, coop=0, over=dict(sequence_model="GRU"), host=False)
case("gru_fbn2_rt", [P(0, 257, 9)], B=1, coop=0, over=dict(sequence_model="GRU", fb_num_neighbors=2), host=False)             # (the GRU at K = 64)
case("gru_ks16", [P(1, 257, 9, par=16)], B=1, costs="ks16", over=dict(sequence_model="GRU"), host=False, differs_from="gru_rt")
case("tcn_f161_b1", kernels=("sub-band TCN",), B=1, T=8, F=161, over=dict(sequence_model="TCN"), costs=None)      # (the oracle's TCN costs 25 ms per sequence)
case("output3_generic", kernels=("lstm2_generic_kernel",), B=1, T=10, over=dict(output_size=3))          # (the tuned kernels write two outputs)
case("tanh_output", [P(9, 514, 17, par=32)], over=dict(sb_output_activate_function="Tanh"))
# 9. all four norms on a row-tile path and on a column split; the cumulative ones across the 256-frame chunks of sb_cumulative_kernel
for _n in NORMS:
    case(f"norm_rt_{_n}", [P(0, 514, 17)], coop=0, over=dict(norm_type=_n), profile="default")
    case(f"norm_cw32_{_n}", [P(9, 514, 17, par=32)], over=dict(norm_type=_n), profile="default", differs_from=f"norm_rt_{_n}")
for _n in CUMULATIVE:
    for _tp in (255, 256, 257):
        case(f"cum_chunks_{_n}_tp{_tp}", [P(8, 257, 9)], B=1, T=_tp - 2, over=dict(norm_type=_n))
# 10. drop band ("parity": 2 groups at B = 3 and 4, 3 groups at B = 4; no bin count here is a multiple of its group count) and the
#     sb_offline_stats_kernel grids of B = 1, 2, 4, 8 in full mode
case("parity_b3", [P(8, 320, 10), P(1, 64, 2, par=8)], B=3, mode="parity")
case("parity_b4", [P(9, 512, 16, par=32)], B=4, mode="parity", profile="default")
case("parity_b4_three_groups_rt", [P(0, 340, 11)], B=4, mode="parity", over=dict(num_groups_in_drop_band=3), coop=0)
case("parity_b4_three_groups", [P(8, 320, 10), P(1, 20, 1, par=8)], B=4, mode="parity", over=dict(num_groups_in_drop_band=3),
     differs_from="parity_b4_three_groups_rt")
case("parity_f161_b3", [P(8, 240, 8)], B=3, F=161, mode="parity", over=dict(norm_type="cumulative_layer_norm"))
case("full_b1", [P(8, 257, 9)], B=1)
case("full_b2", [P(9, 514, 17, par=32)], profile="default")
case("full_b4", [P(9, 1028, 33, par=64)], B=4, T=10, over=dict(norm_type="offline_gaussian_norm"))
case("full_b8", [P(9, 2048, 64, par=96), P(1, 8, 1, par=8)], B=8, T=8, over=dict(norm_type="offline_gaussian_norm"))
# 11. ragged batches: B = 4, lengths[b] + look_ahead one below, at and one above 16 and 32 (8 is the shortest legal clip), 40-frame buffer
RAGGED_T = 40
RAGGED_LENGTHS = edge_lengths(RAGGED_T, 2, 8, edges=(8, 16, 32))
assert RAGGED_LENGTHS == [8, 13, 14, 15, 29, 30, 31, 40]
for _n in ("offline_laplace_norm", "cumulative_layer_norm"):
    case(f"ragged_rt_{_n}", [P(0, 1028, 33)], B=4, T=RAGGED_T, lengths=RAGGED_LENGTHS, coop=0, over=dict(norm_type=_n))
    case(f"ragged_cw64_{_n}", [P(9, 1028, 33, par=64)], B=4, T=RAGGED_T, lengths=RAGGED_LENGTHS, over=dict(norm_type=_n),
         differs_from=f"ragged_rt_{_n}")
# 12. the original FullSubNet (32 inputs, one fb branch, att_mag = the padded magnitude)
case("fsn_b1", [P(8, 257, 9)], model="fsn", B=1)
case("fsn_b3_rt", [P(0, 771, 25)], model="fsn", B=3, T=10, coop=0)
case("fsn_b3", [P(9, 672, 21, par=32), P(1, 99, 4, par=8)], model="fsn", B=3, T=10)
case("fsn_b3_parity", [P(8, 320, 10), P(1, 64, 2, par=8)], model="fsn", B=3, T=10, mode="parity", profile="default")
# 13. other edges
case("look_ahead0", [P(9, 514, 17, par=32)], over=dict(look_ahead=0))
case("look_ahead3", [P(9, 514, 17, par=32)], T=21, over=dict(look_ahead=3), profile="default")
case("eca_subband2", [P(8, 257, 9)], B=1, over=dict(channel_attention_model="ECA", subband_num=2))


def host_plan(c, lib_plan):
    """The case's plan by the host planner: lib_plan(rows, cus, hidden, gru, coop, costs) -> [(kind, rows, tiles, ex, par, rpg)]."""
    costs = TABLES[c["costs"]] if c["costs"] else None
    return lib_plan(rows_of(c), c["cus"] or 256, 384, 0, 1 if c["coop"] else 0, costs)
