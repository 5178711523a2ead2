"""`kmertools unitigs --pop-bubbles` on the CPU: the help text names the flags, the new file, its ten fields, the defaults and the
rule; --bubble-nodes is refused without --pop-bubbles and values out of range are refused, exit 2 with a clap-style message
before any device is opened or the directory is made; --clip-rounds passes with --pop-bubbles alone; the binding declares the
calls.  And the reference the GPU tests compare against (tests/bubble_ref.py): it reproduces the worked answers of
tests/golden/bubble_known.json, keeps its assertions (the definition and the per-thread search agree, one member of every
class stays, the invariant of the union of tip and bubble marks - asserted inside every call) over a few hundred random small
tables (k = 2..7 and 9, alphabets of two letters, circularised genomes, hairpins, min_count 1 and 2, tips on and off), its
array form agrees with its string form, and the two-haplotype recipe of the GPU tests is not vacuous."""
import functools
import json
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import bubble_ref as br  # noqa: E402
import graph_ref as gr  # noqa: E402
import test_ctr_clip_tips_cli_args as tca  # noqa: E402  (its cli fixture, run() and random_reads())
import tip_ref as tr  # noqa: E402
import unitig_link_ref as lr  # noqa: E402
import unitig_ref as ur  # noqa: E402

cli = tca.cli
run = tca.run
FASTA = ">a\nACGTACGTACGTACGTACGTACGTACGTAAACCCGGGTTT\n"


def test_unitigs_help_names_the_bubble_flags(cli):
    for h in ("--help", "-h"):
        r = run(cli, "unitigs", h)
        assert r.returncode == 0
        for text in ("--pop-bubbles", "--bubble-nodes <N>", "[default: 2k]", "unitigs.simplify.stats", "rounds, tips, tip_nodes, isolated, isolated_nodes",
                     "popped, popped_nodes, bubbles", "occurrences", "converged", "(needs --pop-bubbles)", "(needs --clip-tips or --pop-bubbles)",
                     "exactly one link at either end", "highest mean count", "--clip-tips", "unitigs.clip.stats"):
            assert text in r.stdout, text


@pytest.mark.parametrize("extra, what, needs", [
    (("--bubble-nodes", "5"), "--bubble-nodes", "--pop-bubbles"),
    (("--clip-tips", "--bubble-nodes", "5"), "--bubble-nodes", "--pop-bubbles"),
    (("--gfa", "--bubble-nodes", "40", "--links"), "--bubble-nodes", "--pop-bubbles"),
    (("--pop-bubbles", "--tip-nodes", "5"), "--tip-nodes", "--clip-tips"),
    (("--pop-bubbles", "--drop-isolated"), "--drop-isolated", "--clip-tips"),
    (("--clip-rounds", "3"), "--clip-rounds", "--clip-tips"),
])
def test_bubble_flags_need_their_switch(cli, tmp_path, extra, what, needs):
    fa, out = tmp_path / "a.fa", tmp_path / "out"
    fa.write_text(FASTA)
    r = run(cli, "unitigs", "-i", fa, "-o", out, "-k", "15", *extra)
    assert r.returncode == 2, r.stderr
    assert r.stderr.startswith("error: the argument '%s' requires '%s'" % (what, needs)), r.stderr
    assert "For more information, try '--help'." in r.stderr
    assert not out.exists()


@pytest.mark.parametrize("extra, what", [
    (("--pop-bubbles", "--bubble-nodes", "0"), "--bubble-nodes"),
    (("--pop-bubbles", "--bubble-nodes", "2147483647"), "--bubble-nodes"),
    (("--pop-bubbles", "--bubble-nodes", "many"), "--bubble-nodes"),
    (("--pop-bubbles", "--clip-rounds", "0"), "--clip-rounds"),
    (("--pop-bubbles", "--clip-rounds", "1025"), "--clip-rounds"),
    (("--pop-bubbles", "yes"), "yes"),
    (("--pop-bubbles", "--stats-only", "--gfa"), "--stats-only"),
])
def test_bubble_flag_values_out_of_range(cli, tmp_path, extra, what):
    fa, out = tmp_path / "a.fa", tmp_path / "out"
    fa.write_text(FASTA)
    r = run(cli, "unitigs", "-i", fa, "-o", out, "-k", "15", *extra)
    assert r.returncode == 2 and r.stderr.startswith("error: ") and what in r.stderr, r.stderr
    assert not out.exists()


@pytest.mark.parametrize("extra", [("--pop-bubbles", "--clip-rounds", "3"), ("--pop-bubbles", "--bubble-nodes", "2147483646"),
                                   ("--pop-bubbles", "--clip-tips", "--drop-isolated", "--tip-nodes", "4", "--bubble-nodes", "1")])
def test_bubble_flags_that_pass(cli, tmp_path, extra):
    """the arguments are taken: the run gets as far as the device (and, where there is one, through)"""
    fa, out = tmp_path / "a.fa", tmp_path / "out"
    fa.write_text(FASTA)
    r = run(cli, "unitigs", "-i", fa, "-o", out, "-k", "15", *extra)
    assert r.returncode in (0, 101) and not r.stderr.startswith("error: "), r.stderr
    assert out.exists()


def test_the_binding_declares_the_calls():
    from kmertools_amd import _lib, device
    for name in ("unitig_bubbles", "unitig_bubbles_device", "simplify"):
        assert callable(getattr(device.Counter, name)), name
    assert (device.TIP_TIP, device.TIP_ISOLATED, device.BUBBLE_POP) == (br.TIP, br.ISOLATED, br.POP) == (1, 2, 4)
    assert device.SIMPLIFY_STATS_NAMES == br.STATS and len(br.STATS) == 10
    for name in ("kt_ctr_unitig_bubbles", "kt_ctr_simplify"):
        assert name in _lib.SYMBOLS
    header = (ROOT / "include" / "kmertools_hip.h").read_text()
    for text in ("#define KT_BUBBLE_POP 4", "#define KT_BUBBLE_TALLY 4", "#define KT_SIMPLIFY_STATS 12"):
        assert text in header, text
    assert (_lib.KT_BUBBLE_POP, _lib.KT_BUBBLE_TALLY, _lib.KT_SIMPLIFY_STATS) == (4, 4, 12)


# ---- the reference ----------------------------------------------------------------------------------------------------------

KNOWN = json.loads((ROOT / "tests" / "golden" / "bubble_known.json").read_text())["cases"]
CLIP_KNOWN = json.loads((ROOT / "tests" / "golden" / "clip_tips_known.json").read_text())["cases"]


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: c["name"])
def test_reference_reproduces_the_worked_answers(case):
    k, mb, mt = case["k"], case["max_bubble_nodes"], case["max_tip_nodes"]
    table = gr.count_strings(case["reads"], k)
    assert [u[0] for u in ur.unitigs(table, k)] == case["unitigs"]
    for tips, pre in ((0, ""), (mt, "tip_")):
        red, s, rounds = br.simplify(table, k, tips, mb)
        assert rounds == case[pre + "rounds"] and s == case[pre + "stats"]
        assert [u[0] for u in ur.unitigs(red, k)] == case[pre + "survivors"]
        assert s[9] == 0 and s[0] == len(rounds) - 1 and s[10:] == [0, 0]
        assert sum(table.values()) - sum(red.values()) == s[8] and len(table) - len(red) == s[2] + s[4] + s[6]
        assert tips or s[1:5] == [0, 0, 0, 0]


def test_the_worked_answers_cover_the_rule():
    by = {c["name"]: c for c in KNOWN}
    assert len(KNOWN) == 12

    def popped(name, r=0, pre=""):
        return [u for u, m in zip(by[name]["unitigs"], by[name][pre + "rounds"][r]) if m == br.POP]

    def branches(name):
        c = by[name]
        us, ls = lr.links(gr.count_strings(c["reads"], c["k"]), c["k"])
        return us, ls, br.branches_of([u[3] for u in us], [bool(u[2] & ur.CIRCULAR) for u in us], ls, c["max_bubble_nodes"])

    snp = by["SNP, unequal coverage"]
    assert popped("SNP, unequal coverage") == ["CATTTTGAC"] and snp["survivors"] == [snp["reads"][0]]  # the weaker branch; one unitig is left
    us, _, b = branches("SNP, unequal coverage")
    assert sorted(b) == [0, 3] and us[0][1] * us[3][3] < us[3][1] * us[0][3]
    assert popped("SNP, equal coverage") == ["CATTGTGAC"] and by["SNP, equal coverage"]["unitigs"][0] == "CATTTTGAC"  # a tie: the lower number stays
    us, _, b = branches("SNP, equal coverage")
    assert us[0][1] * us[3][3] == us[3][1] * us[0][3]
    three = by["three parallel branches"]
    assert len(popped("three parallel branches")) == 2 and three["stats"][5:8] == [2, 10, 1] and len(three["survivors"]) == 1
    indel = by["indel"]
    assert popped("indel") == ["CATTTGAC"] and indel["stats"][5:8] == [1, 4, 1]
    us, _, b = branches("indel")
    assert sorted(us[u][3] for u in b) == [4, 5]  # branches of different n
    long_ = by["a branch one node too long"]
    assert long_["reads"] == snp["reads"] and long_["max_bubble_nodes"] == 4 and long_["rounds"] == [[0, 0, 0, 0]]
    hair = by["the tip cases' bubble"]
    clip = next(c for c in CLIP_KNOWN if c["name"] == "bubble")
    assert hair["reads"] == clip["reads"] and hair["k"] == clip["k"] == 5 and hair["unitigs"] == clip["unitigs"]
    assert hair["rounds"] == [[0] * 5] and "AAGCT" in hair["unitigs"]  # the hairpin node gives the two paths different anchors
    assert not any(br.POP in r for r in hair["tip_rounds"]) and hair["tip_stats"][:5] == clip["stats"][:5]
    hidden = by["a bubble behind a tip"]
    assert hidden["rounds"] == [[0] * 6] and hidden["stats"] == [0] * 12  # never with bubbles alone
    assert hidden["tip_rounds"][0].count(br.TIP) == 1 and br.POP not in hidden["tip_rounds"][0]
    assert hidden["tip_rounds"][1].count(br.POP) == 1 and hidden["tip_stats"][0] == 2 and len(hidden["tip_survivors"]) == 1
    _, _, b = branches("two branches that leave a unitig and come back to it")
    assert len(b) == 2 and all(x == y ^ 1 for x, y in b.values())
    assert len(popped("two branches that leave a unitig and come back to it")) == 1
    _, _, b = branches("both ends of a branch on the same oriented end")
    assert len(b) == 2 and all(x == y for x, y in b.values())
    assert len(popped("both ends of a branch on the same oriented end")) == 1
    us, ls, b = branches("a cycle and a self-linked homopolymer")
    assert not b and ls[0] == [0] and ls[1] == [1] and us[1][2] & ur.CIRCULAR and not us[0][2] & ur.CIRCULAR
    for name in ("a palindromic node for an anchor", "a palindromic node beside a bubble"):
        assert by[name]["k"] % 2 == 0 and "AACGTT" in by[name]["unitigs"]
    us, ls, b = branches("a palindromic node for an anchor")
    p = by["a palindromic node for an anchor"]["unitigs"].index("AACGTT")
    assert not b and p == 2 and sorted(map(len, ls[0:2])) == [1, 2] and set(ls[0] + ls[1]) >= {2 * p, 2 * p + 1}  # linked under both signs: no branch
    assert by["a palindromic node for an anchor"]["rounds"] == [[0] * 5]
    assert by["a palindromic node beside a bubble"]["stats"][5:8] == [1, 6, 1]
    # stopped after one round the call says so, and a second call finishes the job
    table = gr.count_strings(hidden["reads"], hidden["k"])
    red, s, _ = br.simplify(table, hidden["k"], hidden["max_tip_nodes"], hidden["max_bubble_nodes"], max_rounds=1)
    assert s[0] == 1 and s[9] == 1 and s[1] == 1 and s[5] == 0
    red2, s2, _ = br.simplify(red, hidden["k"], hidden["max_tip_nodes"], hidden["max_bubble_nodes"])
    assert s2[0] == 1 and s2[9] == 0 and s2[5] == 1 and [u[0] for u in ur.unitigs(red2, hidden["k"])] == hidden["tip_survivors"]


def test_simplify_without_bubbles_is_clip():
    for case in CLIP_KNOWN:
        table = gr.count_strings(case["reads"], case["k"])
        for drop in (False, True):
            red, s, rounds = br.simplify(table, case["k"], case["max_tip_nodes"], 0, 8, drop)
            wred, ws, wrounds = tr.clip(table, case["k"], case["max_tip_nodes"], 8, drop)
            assert red == wred and rounds == wrounds and s[:5] + [s[8], s[9]] == ws[:7] and s[5:8] == [0, 0, 0]


def random_reads(rng, k, letters):
    """the tip tests' reads, and for bubbles: copies of some reads with a substitution or a missing base in their middle"""
    reads = tca.random_reads(rng, k, letters)
    L = list(letters)
    for r in list(reads[:4]):
        if len(r) >= 2 * k and rng.random() < 0.9:
            p = int(rng.integers(k - 1, len(r) - k + 1))
            reads.append(r[:p] + (L[int(rng.integers(0, len(L)))] if rng.random() < 0.7 else "") + r[p + 1:])
            if rng.random() < 0.5:  # a third path between the same two points
                reads.append(r[:p] + L[int(rng.integers(0, len(L)))] + r[p + 1:])
    return reads


SWEEP_KS = (2, 3, 4, 5, 6, 7, 9)


@functools.lru_cache(maxsize=None)
def sweep(k):
    """48 random tables at k through the reference (which asserts what its docstring lists) -> what they held.  Cached: the
    test of one k and the test of what all of them saw share a run, in whatever order and selection they are run."""
    seen = dict(popped=0, bubbles=0, ties=0, big_classes=0, two_rounds=0, both_marks=0, later_pop=0, tables=0)
    rng = np.random.default_rng(7300 + k)
    for trial in range(24):
        table = gr.count_strings(random_reads(rng, k, "ACGT" if trial % 3 else "AC"), k)
        for lo in (1, 2):
            for mt in (0, k, 2 * k):
                for mb in (1, k, 2 * k):
                    us, ls, m, bt, tt = br.marks(table, k, mb, mt, lo)
                    n, c = [u[3] for u in us], [u[1] for u in us]
                    assert len(m) == len(us) and bt[0] == m.count(br.POP) and tt[0] == m.count(br.TIP)
                    if us:  # the array form, on the arrays the library would fill
                        off = np.cumsum([0] + [len(u[0]) for u in us]).astype(np.uint64)
                        loff, lto = lr.as_arrays(ls)
                        m2, t2 = br.marks_of_arrays(off, np.array(c, np.uint64), np.array([u[2] for u in us], np.uint32), loff, lto, k, mb, mt)
                        assert m2.dtype == np.uint8 and m2.tolist() == m and t2.tolist() == bt
                    b = br.branches_of(n, [bool(u[2] & ur.CIRCULAR) for u in us], ls, mb)
                    classes, _ = br.by_definition(n, c, b)
                    seen["popped"] += bt[0]
                    seen["bubbles"] += bt[2]
                    seen["big_classes"] += any(len(g) >= 3 for g in classes)
                    seen["ties"] += any(x != y and c[x] * n[y] == c[y] * n[x] for g in classes for x in g for y in g)
                    seen["both_marks"] += br.POP in m and br.TIP in m
            for mt, drop in ((0, False), (k, False), (k, True)):
                red, s, rounds = br.simplify(table, k, mt, 2 * k, 8, drop, lo)
                assert set(red) <= set(table) and all(red[key] == table[key] for key in red)
                assert all(key in red for key in table if table[key] < lo)  # entries that are no nodes are never touched
                assert len(table) - len(red) == s[2] + s[4] + s[6] and sum(table.values()) - sum(red.values()) == s[8]
                assert s[0] == len(rounds) - (0 if s[9] else 1)
                seen["two_rounds"] += s[0] >= 2
                seen["later_pop"] += any(br.POP in r for r in rounds[1:])
            seen["tables"] += 1
    return seen


@pytest.mark.parametrize("k", SWEEP_KS)
def test_the_reference_keeps_its_assertions(k):
    assert sweep(k)["tables"] == 48


def test_the_sweep_saw_what_it_is_for():
    seen = {name: sum(sweep(k)[name] for k in SWEEP_KS) for name in sweep(SWEEP_KS[0])}
    assert seen["tables"] == 7 * 48, seen
    assert all(seen.values()), seen
    assert seen["popped"] > 200 and seen["bubbles"] > 200, seen


@pytest.mark.parametrize("k", [9, 11, 12])
def test_the_recipe_is_not_vacuous(k):
    """the two-haplotype tables of the GPU tests, 14 at each k: at least 4 popped unitigs each in round one, by the reference
    alone; every one converges within 3 rounds that erase; at every k some pop a bubble only after round one (behind a tip)"""
    later = 0
    for seed in range(14):
        table = gr.count_strings(br.two_haplotypes(1000 * k + seed, k), k)
        _, _, m, bt, tt = br.marks(table, k, 2 * k, k)
        assert bt[0] >= 4 and bt[2] >= 4, (k, seed, bt)
        red, s, rounds = br.simplify(table, k, k, 2 * k)
        assert s[9] == 0 and s[0] <= 3 and s[5] >= bt[0], (k, seed, s)
        later += any(br.POP in r for r in rounds[1:])
    print("k=%d: %d of 14 tables popped something after round one" % (k, later))
    assert later >= 1, (k, later)


def test_simplify_stats_rendering():
    assert br.want_simplify_stats([2, 3, 6, 1, 2, 4, 20, 3, 40, 0, 0, 0]) == \
        b"rounds\t2\ntips\t3\ntip_nodes\t6\nisolated\t1\nisolated_nodes\t2\npopped\t4\npopped_nodes\t20\nbubbles\t3\noccurrences\t40\nconverged\t1\n"
    assert br.want_simplify_stats([1, 0, 0, 0, 0, 1, 5, 1, 5, 1, 0, 0]).endswith(b"converged\t0\n")
