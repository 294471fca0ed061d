"""The LDS bank model of tools/probes/lds_banks.py (CPU): the figures of the LDS table of MI355X_MICROARCH.md on known patterns, and the
sweep step of lqr_mfma16x8.hip on the committed layout constants and on the earlier layout (column stride 8)."""

import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("lds_banks", os.path.join(ROOT, "tools", "probes", "lds_banks.py"))
lds_banks = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lds_banks)


def test_known_patterns():
    # 16 columns at a stride of 8 floats, row q of column i in lane 16 q + i (the value update at stride 8): columns i, i + 4, i + 8,
    # i + 12 share a bank of the 32 -> four-way, 2 x 4 cycles where 2 are conflict-free
    col8 = lambda lane: 8 * (lane & 15) + (lane >> 4)
    assert lds_banks.cycles("ds_read_b32", col8) == (8, 2)
    assert lds_banks.ways("ds_read_b32", col8) == 4
    assert lds_banks.cycles("ds_read_b32", lambda lane: lane) == (2, 2)
    # every lane on one dword: a broadcast, no conflict
    assert lds_banks.cycles("ds_read_b32", lambda lane: 7) == (2, 2)
    # a contiguous 16-byte read: four groups of 16 lanes cover the 64 banks once each
    assert lds_banks.cycles("ds_read_b128", lambda lane: 4 * lane) == (4, 4)
    # 16-byte stores 32 B apart: a group of eight lanes covers banks 0-3, 8-11, 16-19, 24-27 twice
    assert lds_banks.ways("ds_write_b128", lambda lane: 8 * lane) == 2
    assert lds_banks.cycles("ds_write_b128", lambda lane: 8 * lane) == (16, 8)
    assert lds_banks.cycles("ds_write_b128", lambda lane: 4 * lane) == (8, 8)
    assert lds_banks.cycles("ds_write_b64", lambda lane: 2 * lane) == (4, 4)
    assert lds_banks.cycles("ds_write_b32", lambda lane: lane) == (2, 2)
    assert lds_banks.cycles("ds_read_b64", lambda lane: 2 * lane) == (2, 2)
    # masked lanes: half a wave of 16-byte stores is four groups
    assert lds_banks.cycles("ds_write_b128", lambda lane: 4 * lane if lane < 32 else None) == (4, 4)
    # ds_read2_b32 is two dword reads
    assert lds_banks.cycles("ds_read2_b32", lambda lane: (col8(lane), col8(lane) + 4)) == (16, 4)


def test_sweep_step_of_the_earlier_layout():
    res = lds_banks.sweep_step(cols=8, gain_regs=0)
    assert res["cycles"] == 102 and res["free"] == 44
    assert res["conflict"] == 58           # x 3.2768 M instance-steps = 190 M of the 206.0 M cycles of profiles/r12_mfma16x8_pmc_summary.json


def test_sweep_step_of_the_committed_layout():
    c = lds_banks.read_constants()
    res = lds_banks.sweep_step()
    L = res["layout"]
    assert L["cols"] == c["cols"] and L["sweep"] <= L["rollout"] == L["lds"]          # the slice did not grow
    assert res["cycles"] <= (56 if c["gain_regs"] else 64)
    assert lds_banks.sweep_step(gain_regs=0)["cycles"] <= 64
