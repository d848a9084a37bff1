"""The generated code of the hot loops, frozen (VERDICT r04 "next round" item 2).

Rounds 3-4 bought their last 15 % with things no correctness test sees: physical registers pinned in asm constraints, an occupancy hint the
compiler cannot meet chosen for where the scheduler then settles, -amdgpu-sched-strategy=max-ilp, -align-all-nofallthru-blocks=6, -O2 over -O3.
A ROCm point release -- or an innocent edit of a header -- that puts a spill, a scratch access or a few scalar branches back into a round loop
costs 5-10 % and every parity test stays green.  This test compiles the product's translation units to gfx950 assembly with the SHIPPED
flags (__graft_entry__.FLAGS / UNITS; hipcc cross-compiles without a GPU: about 95 s the first time, cached under build/codegen/ by a hash of
sources + flags + compiler version) and asserts on what tools/round_loop_lanes.py, tools/spills_by_loop.py and tools/kernel_resources.py print.

The bounds are the shipped numbers plus a few instructions of slack: they are meant to fail when the code gets worse, and to be tightened
(with a measurement in DESIGN.md) when it gets better."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


@pytest.fixture(scope="module")
def cg():
    import codegen as C
    units = C.compile_units()
    return C, C.resources(units), C.asm_lines(units)


def _round_loop(C, lines, sub):
    name, body = C.kernel_body(lines, sub)
    header = next(h for d, h in C.loop_headers(body) if d == 3)          # replica -> pass -> block -> ROUND
    return C.totals(C.hot_path(body, header)), C.loops(body)


@pytest.mark.parametrize("nlu", [4, 6])          # d = 1024 (the metric, C2) and d = 4096 (C4)
def test_slice8_round_loop(cg, nlu):
    """k_explore_slice8<NLU, 9>: the path from the round loop's header to its back edge holds no spill write, no spill reload and no scratch
    access; its only lane instructions are the chase's five v_readlane; 301 instructions (238 VALU + 53 scalar + 10 LDS) in 8 blocks as shipped."""
    C, res, lines = cg
    t, _ = _round_loop(C, lines, "k_explore_slice8ILi%dELi9E" % nlu)
    assert t["w"] == 0 and t["r"] == 0 and t["scratch"] == 0 and t["m"] == 0, t
    assert t["dyn"] == 5, t                       # the chained chase: one v_readlane per level
    assert t["instructions"] <= 310, t
    assert t["v"] <= 244 and t["s"] <= 58 and t["l"] <= 10, t
    assert t["blocks"] <= 9, t                    # every extra block on the likely path is a branch a lone wave pays ~18-40 cycles for


@pytest.mark.parametrize("nlu", [0, 4, 5])       # d = 2 (C1), d = 1024 (the metric, C2), d = 2048 (the longest rows the fused loop takes)
def test_fused_scan_loop_round_loop(cg, nlu):
    """k_scans_slice8<NLU, 9> (round 5: all the scans of a pte_run_scans call in one launch; the metric runs THIS kernel): the scan loop
    around the body must not cost the round loop anything -- the same 301 instructions in 8 blocks, no spill, no scratch -- and the kernel must
    keep two waves per SIMD's worth of registers (the launcher admits one: 1024 workgroups on 1024 SIMDs)."""
    C, res, lines = cg
    name, body = C.kernel_body(lines, "k_scans_slice8ILi%dELi9E" % nlu)
    header = next(h for d, h in C.loop_headers(body) if d == 4)          # SCAN -> pass -> block -> round
    t = C.totals(C.hot_path(body, header))
    assert t["w"] == 0 and t["r"] == 0 and t["scratch"] == 0 and t["m"] == 0 and t["dyn"] == 5, t
    assert t["instructions"] <= 310 and t["v"] <= 244 and t["s"] <= 58 and t["blocks"] <= 9, t
    r = res["k_scans_slice8<%d, 9>" % nlu]
    assert r["scratch_B_per_lane"] == 0 and r["spilled_vgpr"] == 0 and r["vgpr"] <= 256 and r["waves_per_simd"] >= 2, r
    g = res["k_scans_slice8_generic<%d, 9>" % nlu]
    assert g["scratch_B_per_lane"] == 0 and g["spilled_vgpr"] == 0 and g["waves_per_simd"] >= 2, g


def test_slice8_resources(cg):
    """every instantiation of the default kernel and of its generic twin: no VGPR spill, no scratch, two waves per SIMD (2048 replicas resident)"""
    C, res, _ = cg
    for nlu in range(7):
        for k in ("k_explore_slice8<%d, 9>" % nlu, "k_explore_slice8_generic<%d, 9>" % nlu):
            r = res[k]
            assert r["scratch_B_per_lane"] == 0 and r["spilled_vgpr"] == 0, (k, r)
            assert r["waves_per_simd"] >= 2 and r["vgpr"] <= 200, (k, r)
            assert r["lds_B"] <= 16384, (k, r)


@pytest.mark.parametrize("nlu", [4, 5, 6])
def test_slice8_many_replica_twin(cg, nlu):
    """k_explore_slice8_lds10k (more than 2048 replicas per GPU; the strong-scaling anchor): capped at 128 VGPRs = four waves per SIMD, 10 KB of
    LDS = 16 replicas per CU.  The instantiations for d >= 1024 DO spill 14-16 VGPRs (12-20 B of scratch per lane, the faster side of the A/B in
    DESIGN) -- but not in the round loop: its hot path touches no scratch and writes no spill."""
    C, res, lines = cg
    r = res["k_explore_slice8_lds10k<%d, 9>" % nlu]
    assert r["vgpr"] <= 128 and r["waves_per_simd"] == 4 and r["lds_B"] <= 10240, r
    assert r["scratch_B_per_lane"] <= 24 and r["spilled_vgpr"] <= 18, r
    t, _ = _round_loop(C, lines, "k_explore_slice8_lds10kILi%dELi9E" % nlu)
    assert t["scratch"] == 0 and t["m"] == 0 and t["w"] == 0, t
    assert t["dyn"] == 5 and t["instructions"] <= 385, t


def test_automala_config3_leapfrog_loops(cg):
    """k_explore_automala<2, 2, false, true> (funnel d = 128, the C3 instantiation): every loop below the refresh loop -- the step-size searches
    and the leapfrogs inside them -- is free of spill writes, reloads and scratch, and a leapfrog body stays at <= 470 vector instructions."""
    C, res, lines = cg
    name, body = C.kernel_body(lines, "k_explore_automalaILi2ELi2ELb0ELb1E")
    r = res["k_explore_automala<2, 2, false, true>"]
    assert r["scratch_B_per_lane"] == 0 and r["spilled_vgpr"] == 0 and r["waves_per_simd"] >= 3, r
    inner = {k: L for k, L in C.loops(body).items() if k[0] >= 2}
    assert len(inner) >= 8
    for k, L in inner.items():
        assert L["w"] == 0 and L["r"] == 0 and L["scratch"] == 0, (k, L)
        assert L["v"] <= 470, (k, L)
    assert max(L["v"] for L in inner.values()) >= 400            # the leapfrog bodies are among them (the test looks at the right loops)


def test_fused_automala_loops_keep_the_per_scan_allocation(cg):
    """k_scans_automala / k_scans_automala_wg (C3 runs the second: four chains per workgroup): the body is a CALLED function, so the scan loop's
    own long-lived values never reach the step-size search loops; no VGPR spill in either kernel, one workgroup of four waves per compute unit"""
    C, res, _ = cg
    for k in ("k_scans_automala<2, 2, false>", "k_scans_automala_wg<2, 2, false>"):
        r = res[k]
        assert r["spilled_vgpr"] == 0 and r["waves_per_simd"] >= 1 and r["lds_B"] <= 6656, (k, r)
        assert r["scratch_B_per_lane"] <= 700, (k, r)          # the engine's argument block handed to the called body by reference


def test_ising_word_loop(cg):
    """k_explore_ising_spec<false> (C5: 256 x 256): per 32-site word the likely path is 6 blocks (round 3: 12), 204 VALU + 52 scalar + 4 LDS
    instructions, spill-free; no scratch anywhere in the kernel."""
    C, res, lines = cg
    r = res["k_explore_ising_spec<false>"]
    assert r["scratch_B_per_lane"] == 0 and r["spilled_vgpr"] == 0 and r["waves_per_simd"] >= 4, r
    name, body = C.kernel_body(lines, "k_explore_ising_specILb0E")
    header = next(h for d, h in C.loop_headers(body) if d == 3)          # replica -> sweep -> row -> WORD
    t = C.totals(C.hot_path(body, header))
    assert t["blocks"] <= 6, t
    assert t["w"] == 0 and t["r"] == 0 and t["scratch"] == 0, t
    assert t["instructions"] <= 268 and t["v"] <= 210 and t["s"] <= 58, t


def test_hbm_bound_kernels_resources(cg):
    """k_explore_toy / k_init (the HBM-write-bound kernels): five waves per SIMD with 31 KB of LDS per workgroup; k_init within 12 B,
    k_explore_toy within 20 B of scratch per lane (cold: the reference-chain / recorder epilogue)."""
    C, res, _ = cg
    for nlu in range(7):
        a, b = res["k_explore_toy<%d>" % nlu], res["k_init<%d>" % nlu]
        assert a["scratch_B_per_lane"] <= 20 and a["waves_per_simd"] >= 5 and a["vgpr"] <= 96, a
        assert b["scratch_B_per_lane"] <= 12 and b["spilled_vgpr"] <= 2 and b["waves_per_simd"] >= 5 and b["vgpr"] <= 96, b      # (round 5: the pipelined position slots cost k_init<5, 6> two spilled VGPRs)


def test_swap_kernels_are_light(cg):
    """the DEO swap kernels: full occupancy, no spills (they are launch-latency bound; nothing else should ever show up in them)"""
    C, res, _ = cg
    for k in ("k_swap", "k_swap_stats", "k_swap_decide", "k_boundary_pack", "k_boundary_stats_in", "k_boundary_apply"):
        r = res[k]
        assert r["waves_per_simd"] == 8 and r["scratch_B_per_lane"] == 0 and r["spilled_sgpr"] == 0 and r["spilled_vgpr"] == 0, (k, r)


def test_langevin_mw_kernels(cg):
    """k_explore_langevin_mw / k_scans_langevin_mw (round 6: AutoMALA / MALA at 512 < d <= 1024, four waves per replica): 128 VGPRs = four waves per SIMD = four workgroups per
    compute unit (1024 replicas resident; 39 KB of LDS each: four fit the 160 KB).  Scaled-precision MVN path: the loop of trial leapfrogs (~300 VALU + 150
    scalar + 15 LDS instructions: the one holding the cross-wave exchange) touches no scratch and holds no spill write -- what is spilled (55-68 values) is
    spilled at refresh level.  Funnel path: its evaluation does not fit beside the vectors (124-176 values spilled) and is still fastest at this setting
    (profiles/r06_langevin_mw.txt)."""
    C, res, lines = cg
    for full in ("true", "false"):
        r = res["k_explore_langevin_mw<0, %s>" % full]
        assert r["vgpr"] <= 128 and r["waves_per_simd"] == 4 and r["lds_B"] <= 40960, r
        assert r["spilled_vgpr"] <= 80 and r["scratch_B_per_lane"] <= 340, r
        name, body = C.kernel_body(lines, "k_explore_langevin_mwILi0ELb%dE" % (1 if full == "true" else 0))
        loops = {k: L for k, L in C.loops(body).items() if k[0] >= 2}
        trial = [L for L in loops.values() if L["l"] >= 10 and 250 <= L["v"] <= 340]          # (the 437-VALU loops are wave_randn_block's: reference chain, sequential momentum)
        assert len(trial) == 1, loops
        t = trial[0]
        assert t["scratch"] == 0 and t["w"] == 0 and t["r"] <= 2 and t["v"] <= 320 and t["s"] <= 170, (full, t)
        for k, L in loops.items():
            assert L["scratch"] <= 2, (full, k, L)                          # nothing at any loop level below the refresh reloads more than a value or two from scratch
        # the scan loop's body (k_scans_langevin_mw calls it): the SAME trial loop -- it reads the kernel-argument segment itself (scalar loads); handed a reference
        # to the caller's copies it issued 4x the vector memory reads and ran at 0.97 instead of 0.65 ms per scan
        s_ = res["k_scans_langevin_mw<0, %s>" % full]
        assert s_["vgpr"] <= 128 and s_["waves_per_simd"] == 4 and s_["lds_B"] <= 40960, s_
        cname, cbody = C.kernel_body(lines, "langevin_mw_body_calledILi0ELb%dELb1E" % (1 if full == "true" else 0))
        cloops = {k: L for k, L in C.loops(cbody).items() if k[0] >= 2}
        ctrial = [L for L in cloops.values() if L["l"] >= 10 and 250 <= L["v"] <= 340]
        assert len(ctrial) == 1, cloops
        assert ctrial[0]["scratch"] <= (0 if full == "true" else 2) and ctrial[0]["w"] == 0 and ctrial[0]["r"] <= 2 and ctrial[0]["v"] <= 320 and ctrial[0]["s"] <= 170, (full, ctrial[0])
        assert sum("flat_load" in l for l in cbody) == 0 and sum("s_load_dword" in l for l in cbody) >= 20, cname     # the engine's fields: scalar loads from the constant address space
        f = res["k_explore_langevin_mw<2, %s>" % full]
        assert f["vgpr"] <= 128 and f["waves_per_simd"] == 4 and f["lds_B"] <= 40960 and f["spilled_vgpr"] <= 100, f
        # the funnel's trial loop: its exp / log / reciprocal (wave 0's funnel_scale) are a CALLED function -- inlined, their ~20 polynomial coefficients are hoisted out
        # of the loop, spilled and read back from scratch one by one behind an s_waitcnt each: 17 exposed round trips per trial, 1.60 instead of 1.20 ms per scan
        fname, fbody = C.kernel_body(lines, "k_explore_langevin_mwILi2ELb%dE" % (1 if full == "true" else 0))
        ftrial = [L for k, L in C.loops(fbody).items() if k[0] >= 2 and L["l"] >= 20 and 500 <= L["v"] <= 760]
        assert len(ftrial) == 1, C.loops(fbody)
        assert ftrial[0]["scratch"] <= 6 and ftrial[0]["w"] <= 2, (full, ftrial[0])
    # the one-wave kernels with sixteen blocks per lane are gone from the product build (their SliceSampler instantiation, which does not spill, stays)
    assert [k for k in res if k.startswith("k_explore_automala<16,")] == ["k_explore_automala<16, 2, true, false>"]
    s16 = res["k_explore_automala<16, 2, true, false>"]
    assert s16["scratch_B_per_lane"] == 0 and s16["spilled_vgpr"] == 0, s16
