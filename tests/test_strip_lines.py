"""Whole-line strips of the fp64 engine without a GPU.

* The rule (flow_list.hpp strip_permuted through tqr_flow_strip_layout): for every plan of 1..6 x 1..6
  tiles and every cap, each tile is found by its reader in the layout the reader's own access expects
  — the panel, an UNMQR element and every head-row access read standard tiles, a TSMQR strip load the
  whole-line layout from step 1 on — and every tile is standard after the last step.
* The map (strip_lane_off / strip_odd_off through tqr_flow_strip_offset): a bijection on the wave's
  block, each store instruction's 64 addresses 8 aligned 128-byte runs.
* The generator: its default output is the committed chain_asm_gen.inc, untouched by the layout; its
  --lines output (the B = 256 statements the engine runs, written by the build) passes the generator's
  simulation of the counted waits and the gfx950 hazard audit, differs from the committed statements
  in the strip accesses' address operands only, and takes them in the form the map assumes.
"""
import importlib.util
import pathlib
import re

import numpy as np
import pytest

PKG = pathlib.Path(__file__).resolve().parent.parent / "gpu-tiled-qr-decomposition_amd"
F64 = 1
T_CHAIN = 4
B = 256


def gen_module():
    spec = importlib.util.spec_from_file_location("gen_chain_asm", PKG / "gen" / "gen_chain_asm.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_reader_finds_its_layout(tqr):
    for p in range(1, 7):
        for q in range(1, 7):
            for steps in range(0, min(p, q) + 1):
                kmax = steps or min(p, q)
                what = (p, q, steps)
                it = tqr.flow_list(p, q, B, F64, steps=steps).astype(np.int64)
                ch = it[(it[:, 0] & 0xff) == T_CHAIN]
                state = {(i, j): 0 for i in range(p) for j in range(q)}  # the caller's matrix: standard
                touched = set()
                for k in range(kmax):
                    for i in range(k, p):  # the panel (GEQRT, TSQRT) reads and writes standard tiles
                        assert state[(i, k)] == 0, (what, "panel", i, k)
                    nxt = dict(state)
                    for ts, l, j, kk in ch[(ch[:, 3] & 0xffff) == k]:
                        seg, i0, i1 = int(kk) >> 16, int(l) & 0xffff, int(l) >> 16
                        j = int(j)
                        assert state[(k, j)] == 0, (what, "head rows / UNMQR strip", k, j)
                        assert tqr.strip_layout(p, q, steps, k, j, k) == 0, (what, "head tile stored", k, j)
                        if seg == 0:
                            touched.add((k, j, k))
                        for i in range(i0, i1):
                            assert state[(i, j)] == (1 if k >= 1 else 0), (what, "TSMQR strip load", i, j, k)
                            nxt[(i, j)] = tqr.strip_layout(p, q, steps, i, j, k)
                            touched.add((i, j, k))
                    state = nxt
                assert touched == {(i, j, k) for k in range(kmax) for j in range(k + 1, q) for i in range(k, p)}, what
                assert not any(state.values()), (what, [t for t, v in state.items() if v])


def test_layout_export_rejects_what_no_plan_touches(tqr):
    L = tqr.lib()
    assert L.tqr_flow_strip_layout(4, 4, 0, 3, 3, 0) == 1
    for args in [(4, 4, 0, 3, 3, 3), (4, 4, 2, 3, 3, 2), (4, 4, 0, 0, 3, 1), (4, 4, 0, 4, 3, 0), (4, 4, 0, 3, 1, 1),
                 (4, 4, 0, 3, 4, 0), (4, 4, 5, 3, 3, 0), (0, 4, 0, 0, 1, 0), (4, 4, 0, 3, 3, -1)]:
        assert L.tqr_flow_strip_layout(*args) == -1, args
    for args in [(2, 0, 0, 16384), (0, 32, 0, 16384), (0, 0, 64, 16384), (1, 0, 0, 128), (1, 0, 0, 1 << 24)]:
        assert L.tqr_flow_strip_offset(*args) == -1, args


@pytest.mark.parametrize("ld", [256, 768, 16384, 16400, 776])
def test_map_is_a_bijection_of_whole_lines(tqr, ld):
    col = 8 * ld
    block = {c * col + b for c in range(16) for b in range(0, 2048, 16)}
    gen = gen_module()
    for layout in (0, 1):
        seen = set()
        for p in range(32):
            offs = [tqr.strip_offset(layout, p, lane, ld) for lane in range(64)]
            seen.update(offs)
            if layout == 0:
                assert offs == [(lane & 15) * col + 64 * p + 16 * (lane >> 4) for lane in range(64)]
                continue
            assert offs == [gen.strip_lines_map(p, lane, col) for lane in range(64)]
            # 8 runs of 128 bytes, each written by 8 consecutive lanes in address order
            runs = [offs[8 * r:8 * r + 8] for r in range(8)]
            for r in runs:
                assert r == list(range(r[0], r[0] + 128, 16)), (p, r)
                assert r[0] % col % 128 == 0
                if ld % 16 == 0:
                    assert r[0] % 128 == 0  # (whole cache lines when the columns are whole lines apart)
            assert len({r[0] for r in runs}) == 8
        assert seen == block and len(seen) == 32 * 64, layout


def _macros(text, prefix):
    return dict(re.findall(r'#define (' + prefix + r'_\w+) "((?:[^"\\]|\\.)*)"', text))


def test_generated_statements(tmp_path, monkeypatch):
    """Default output = the committed .inc. --lines output (main() replays every body sequence against
    the in-order vmcnt model: simulate): every strip access is lane offset va0 / va1 + (odd pair: xso /
    xs) + 64 * pair, every head access loff; with those operands put back to loff / 0 each statement is
    the committed one; and each passes the hazard audit alone and looped."""
    from test_asm_hazards import _violations
    gen = gen_module()
    out, outl = tmp_path / "chain_asm_gen.inc", tmp_path / "chain_asm_lines_gen.inc"
    monkeypatch.setattr("sys.argv", ["gen_chain_asm.py", str(out)])
    gen.main()
    text = (PKG / "csrc" / "chain_asm_gen.inc").read_text()
    assert out.read_text() == text
    monkeypatch.setattr("sys.argv", ["gen_chain_asm.py", "--lines", str(outl)])
    gen.main()
    std, lines = _macros(text, "TQR_CHAIN_ASM"), _macros(outl.read_text(), "TQR_CHAIN_ASML")
    acc = re.compile(r"buffer_(load|store)_dwordx4 v\[(\d+):\d+\], %\[(\w+)\], %\[(\w+)\], (\S+) offen(?: offset:(\d+))?")
    # (strip stores, strip loads) per statement: the hand-overs store 32 row pairs and load all 32 or the
    # first two (late loads, the other 30 in the next element's first body); an UNMQR body stores the 4
    # pairs of the group before it, its hand-over the last 8
    want = {"HANDOVER": (32, 32), "HANDOVERL": (32, 2), "XIN": (0, 30), "UHANDOVER": (8, 32), "UHANDOVERL": (8, 2),
            "STRIP_LOAD": (0, 32), "U1": (4, 0), "U2": (4, 0), "U3": (4, 0), "U4": (4, 0), "U5": (4, 0), "U6": (4, 0)}
    assert set(lines) == {f"TQR_CHAIN_ASML_{n}_B256" for n in want}
    bind = {"vz": "v1", "vx": "v2", "vt": "v3", "vl16": "v4", "loff": "v5", "va0": "v6", "va1": "v7", "svsrc": "s[2:3]",
            "stsrc": "s[4:5]", "sdst": "s6", "sw": "s7", "hrs": "s[8:11]", "goff": "s12", "hsc": "s13", "xout": "s[16:19]",
            "xin": "s[20:23]", "hnx": "s[24:27]", "m0s": "s28", "st": "s29", "xso": "s30", "xs": "s31"}
    for name in want:
        stmt = lines[f"TQR_CHAIN_ASML_{name}_B256"]
        nst = nld = 0
        for kind, reg, voff, rsrc, soff, imm in acc.findall(stmt.replace("\\n\\t", "\n")):
            imm = int(imm or 0)
            if rsrc in ("hrs", "hnx"):
                assert voff == "loff", (name, rsrc)
                continue
            pair = (int(reg) - gen.X0) // 4
            assert rsrc == ("xout" if kind == "store" else "xin") and imm == 64 * pair, (name, reg)
            assert voff == ("va0" if kind == "store" else "va1"), (name, reg)
            assert soff == (("%[xso]" if kind == "store" else "%[xs]") if pair & 1 else "0"), (name, reg)
            nst, nld = nst + (kind == "store"), nld + (kind == "load")
        assert (nst, nld) == want[name], name
        back = stmt.replace("%[va0]", "%[loff]").replace("%[va1]", "%[loff]").replace("%[xso]", "0").replace("%[xs]", "0")
        assert back == std[f"TQR_CHAIN_ASM_{name}_B256"], name
        if name != "STRIP_LOAD":
            body = [l.strip() for l in re.sub(r"%\[(\w+)\]", lambda m: bind[m.group(1)], stmt).split("\\n\\t") if l.strip()]
            alone = ["<asm>"] + body + ["</asm>"]
            assert not _violations(alone), (name, _violations(alone)[:3])
            looped = [".LBB0_9:"] + alone + ["s_cbranch_scc1 .LBB0_9"]
            assert not _violations(looped), (name, _violations(looped)[:3])
