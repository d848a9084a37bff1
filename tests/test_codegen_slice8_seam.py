"""The seam between the doubling block and the shrinkage block of the default SliceSampler kernel after round 9 (pte_slice8.hpp).

The nine shrinkage draws of a hypothesis are requested as soon as the doubling block has restored EXEC -- their address is advanced by the
doubling steps themselves -- so that the LDS round trip runs under the block's last compare, the part of the round that does not depend on
lane 0's out-of-line doubling (the margin, the isapprox threshold, the draw count, "is this coordinate in the block"), the scalar bit test
on the compare and the not-taken branch.  The shrinkage block then waits for the reads one at a time, as its steps need them.

The compiler does not know that the registers the reads return into are pending (the reads live in an asm statement), so what holds the
scheme together is checked here on the generated code of k_scans_slice8<4, 9> -- the kernel the metric runs -- and k_explore_slice8<4, 9>:
where the reads stand, that nothing names their registers before the wait that covers them, that nothing else on the likely path uses the
counter the waits look at (no scalar-memory load: those return out of order), and the size of the path, recorded in
profiles/r09_slice8_round_loop.txt (tools/round_loop_lanes.py k_scans_slice8ILi4ELi9E).  Same source of truth as
tests/test_codegen_slice8_round.py: tools/codegen.py compiles the product's translation units with the shipped flags (cached under
build/codegen/)."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")

SLACK = 4
N_DRAWS = 9                      # PTE_S8_BS
KERNELS = [("k_scans_slice8<4, 9>", "k_scans_slice8ILi4ELi9E", 4), ("k_explore_slice8<4, 9>", "k_explore_slice8ILi4ELi9E", 3)]


def _recorded():
    text = open(os.path.join(ROOT, "profiles", "r09_slice8_round_loop.txt")).read()
    assert "k_scans_slice8<4, 9>" in text
    return int(re.search(r"# HOT path per round: .* = (\d+) instructions in (\d+) blocks", text).group(1))


@pytest.fixture(scope="module")
def cg():
    import codegen as C
    units = C.compile_units()
    return C, C.resources(units), C.asm_lines(units)


@pytest.fixture(scope="module", params=KERNELS, ids=[k[0] for k in KERNELS])
def hot(cg, request):
    """the likely path of the round loop: (kernel, its blocks, [(index of the block, instruction)] in layout order)"""
    C, res, lines = cg
    kernel, sub, depth = request.param
    name, body = C.kernel_body(lines, sub)
    header = next(h for d, h in C.loop_headers(body) if d == depth)
    path = C.hot_path(body, header)
    return kernel, path, [(i, t) for i, b in enumerate(path) for t in b["text"]]


def _vregs(text):
    """the vector registers an instruction names"""
    out = set()
    for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", text):
        out.update(range(int(a), int(b) + 1))
    out.update(int(a) for a in re.findall(r"\bv(\d+)\b", text))
    return out


def _sregs(text):
    out = set()
    for a, b in re.findall(r"\bs\[(\d+):(\d+)\]", text):
        out.update(range(int(a), int(b) + 1))
    out.update(int(a) for a in re.findall(r"\bs(\d+)\b", text))
    return out


def _seam(flat):
    """positions, in the flattened path, of: the last narrowing compare of the doubling block, the reads of the shrinkage draws behind it, the
    conditional branch that follows the doubling block, the first narrowing compare of the shrinkage block"""
    dbl = [k for k, (_, t) in enumerate(flat) if t.startswith("v_cmpx_gt_f64")]
    shr = [k for k, (_, t) in enumerate(flat) if t.startswith("v_cmpx_ngt_f64")]
    assert len(shr) == N_DRAWS and dbl and dbl[-1] < shr[0], (dbl, shr)
    branch = next(k for k in range(dbl[-1], len(flat)) if flat[k][1].startswith("s_cbranch"))
    reads = [k for k in range(dbl[-1], shr[0]) if flat[k][1].startswith("ds_read")]
    return dbl[-1], reads, branch, shr


def test_shrinkage_block_holds_no_lds_read(hot):
    """the nine v_cmpx_ngt_f64 of the shrinkage stand in ONE block, and that block reads nothing from LDS: its draws were requested before"""
    kernel, path, flat = hot
    _, _, _, shr = _seam(flat)
    blocks = set(flat[k][0] for k in shr)
    assert len(blocks) == 1, blocks
    text = path[blocks.pop()]["text"]
    assert not [t for t in text if t.startswith("ds_read")], [t for t in text if t.startswith("ds_")]


def test_draws_are_requested_before_the_branch(hot):
    """four ds_read2_b64 and one ds_read_b64 -- u[0..8], one address register, ascending offsets, consecutive registers -- behind the last
    doubling step, in the doubling block, ahead of the conditional branch that sends lane 0 on"""
    kernel, path, flat = hot
    last_step, reads, branch, shr = _seam(flat)
    assert len(reads) == (N_DRAWS + 1) // 2, [flat[k][1] for k in reads]
    assert all(last_step < k < branch for k in reads), (last_step, reads, branch)
    assert len(set(flat[k][0] for k in reads + [last_step, branch])) == 1            # one basic block
    ops = [flat[k][1] for k in reads]
    assert [o.split()[0] for o in ops] == ["ds_read2_b64"] * (N_DRAWS // 2) + ["ds_read_b64"] * (N_DRAWS % 2), ops
    assert len(set(re.match(r"\S+ v\[\d+:\d+\], (v\d+)", o).group(1) for o in ops)) == 1, ops
    draws, regs = [], []
    for o in ops:
        m = re.search(r"offset0:(\d+) offset1:(\d+)", o)
        draws += [int(m.group(1)), int(m.group(2))] if m else [int(re.search(r"offset:(\d+)", o).group(1)) // 8]
        a, b = map(int, re.match(r"\S+ v\[(\d+):(\d+)\]", o).groups())
        regs += list(range(a, b + 1))
    assert draws == list(range(draws[0], draws[0] + N_DRAWS)), ops
    assert regs == list(range(regs[0], regs[0] + 2 * N_DRAWS)), ops
    # EXEC is whole again when they are issued: the doubling block's restore stands between its last step and the first read
    assert any(re.match(r"s_mov_b64 exec, s\[", flat[k][1]) for k in range(last_step, reads[0])), [flat[k][1] for k in range(last_step, reads[0])]


def test_preamble_stands_between_the_compare_and_its_test(hot):
    """at least eight VALU instructions between the v_cmp that writes the "still needs doubling" mask and the first scalar instruction that
    reads it (a lone wave waits ~30 cycles for a VALU-written SGPR; eight instructions are ~36 cycles of issue)"""
    kernel, path, flat = hot
    last_step, reads, branch, shr = _seam(flat)
    cmp_at = next(k for k in range(last_step, branch) if re.match(r"v_cmp_gt_f64_e64 s\[\d+:\d+\], 0, v\[", flat[k][1]))
    mask = _sregs(flat[cmp_at][1].split(",")[0])
    use_at = next(k for k in range(cmp_at + 1, len(flat)) if flat[k][1].startswith("s_") and _sregs(flat[k][1]) & mask)
    assert use_at <= branch, (flat[use_at][1], flat[branch][1])                      # ... and that reader is the bit test the branch goes by
    assert flat[use_at][1].startswith("s_bitcmp"), flat[use_at][1]
    valu = [flat[k][1] for k in range(cmp_at + 1, use_at) if flat[k][1].startswith("v_")]
    print(kernel, len(valu), "VALU between the compare and its bit test")
    assert len(valu) >= 8, valu
    assert not any(_sregs(v) & mask for v in valu), valu


def test_nothing_names_a_pending_register(hot):
    """LDS returns in order, so read i of n has landed once lgkmcnt <= n - 1 - i has been waited for.  From its request up to the first such
    wait no instruction names its destination registers (the reads themselves apart): no use, no compiler-made copy, no spill.  The first wait
    of any kind behind the reads stands in the shrinkage block -- what the issue's wording asks for, all five reads at once, is the i = 0 case
    with the registers of every read."""
    kernel, path, flat = hot
    last_step, reads, branch, shr = _seam(flat)
    n = len(reads)
    all_regs = set().union(*[_vregs(flat[k][1].split(",")[0]) for k in reads])
    first_wait = next(k for k in range(reads[-1], len(flat)) if re.match(r"s_waitcnt.*lgkmcnt", flat[k][1]))
    assert flat[first_wait][0] == flat[shr[0]][0] and first_wait < shr[0], flat[first_wait]
    for k in range(reads[0], first_wait):
        if k not in reads:
            assert not _vregs(flat[k][1]) & all_regs, flat[k][1]
    for i, at in enumerate(reads):
        regs = _vregs(flat[at][1].split(",")[0])
        k = at + 1
        while True:
            m = re.match(r"s_waitcnt.*lgkmcnt\((\d+)\)", flat[k][1])
            if m and int(m.group(1)) <= n - 1 - i:
                break
            if k not in reads:
                assert not _vregs(flat[k][1]) & regs, (flat[at][1], flat[k][1])
            k += 1
            assert k < shr[-1], "no wait covers %s" % flat[at][1]
        # and it is used behind that wait: the registers are the draws of the steps
        assert any(_vregs(flat[j][1]) & regs for j in range(k, shr[-1])), flat[at][1]


def test_out_of_line_doubling_retires_the_request_first(cg, hot):
    """lane 0's out-of-line doubling is entered with the reads possibly in flight, and it re-reads its draws into the same registers: in
    layout order from the branch's target, an s_waitcnt lgkmcnt(0) -- the one in front of the first use of the path's own first read --
    stands before the first instruction that names them (LDS returns in order: it retires the earlier request as well)"""
    C, res, lines = cg
    kernel, path, flat = hot
    last_step, reads, branch, shr = _seam(flat)
    regs = set().union(*[_vregs(flat[k][1].split(",")[0]) for k in reads])
    target = flat[branch][1].split()[-1]
    sub = next(s for k, s, _ in KERNELS if k == kernel)
    blocks = C.blocks_of(C.kernel_body(lines, sub)[1])
    at = next(i for i, b in enumerate(blocks) if b["name"] == target)
    assert blocks[at] not in path
    waited, named = False, None
    for b in blocks[at:]:
        for t in b["text"]:
            if re.match(r"s_waitcnt.*lgkmcnt\(0\)", t):
                waited = True
            elif _vregs(t) & regs:
                named = t
                break
        if named:
            break
    assert named and named.startswith("ds_read") and waited, (named, waited)


def test_likely_path_uses_the_lgkm_counter_for_lds_only(hot):
    """the staged counts rest on in-order return: no scalar-memory load (out of order, same counter), no message, no vector-memory
    instruction on the likely path of the round"""
    kernel, path, flat = hot
    bad = [t for _, t in flat if re.match(r"s_load|s_buffer_load|s_scratch_load|s_sendmsg|s_memtime|s_memrealtime|global_|flat_|buffer_|scratch_", t)]
    assert not bad, bad


def test_round_loop_size(cg, hot):
    C, res, lines = cg
    kernel, path, flat = hot
    t = C.totals(path)
    print(kernel, t)
    assert t["instructions"] <= _recorded() + SLACK, t
    assert t["l"] == 10 and t["blocks"] <= 8 and t["dyn"] == 5, t
    assert t["w"] == 0 and t["r"] == 0 and t["scratch"] == 0 and t["m"] == 0, t
    assert res[kernel]["spilled_vgpr"] == 0 and res[kernel]["scratch_B_per_lane"] == 0, res[kernel]
