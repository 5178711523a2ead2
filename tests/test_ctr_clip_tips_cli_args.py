"""`kmertools unitigs --clip-tips` on the CPU: the help text names the four flags, the new file and its seven fields; the
flags that need --clip-tips are refused without it, exit 2 with a clap-style message before any device is opened or the
directory is made; the binding declares the calls.  And the reference the GPU tests compare against (tests/tip_ref.py): it
reproduces the worked answers of tests/golden/clip_tips_known.json, keeps its invariant (an end that had links keeps one
among the unmarked unitigs; a marked unitig is short, no cycle and dead at the right ends - asserted inside every call) over a
few hundred random small tables (k = 2..7 and 9, alphabets of two letters, circularised genomes, hairpins, min_count 1 and 2),
and its array form agrees with its string form."""
import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CLI = ROOT / "kmertools_amd" / "bin" / "kmertools"
sys.path.insert(0, str(ROOT / "tests"))
import graph_ref as gr  # noqa: E402
import tip_ref as tr  # noqa: E402
import unitig_link_ref as lr  # noqa: E402
import unitig_ref as ur  # noqa: E402


@pytest.fixture(scope="module")
def cli():
    if not CLI.exists():
        subprocess.check_call(["make", "-C", str(ROOT / "kmertools_amd" / "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return str(CLI)


def run(cli, *args):
    return subprocess.run([cli, *map(str, args)], capture_output=True, text=True, timeout=300)


def test_unitigs_help_names_the_clip_flags(cli):
    for h in ("--help", "-h"):
        r = run(cli, "unitigs", h)
        assert r.returncode == 0
        for text in ("--clip-tips", "--tip-nodes <N>", "--clip-rounds <R>", "--drop-isolated", "unitigs.clip.stats", "rounds, tips, tip_nodes",
                     "isolated, isolated_nodes, occurrences", "converged", "[default: k]", "[default: 8]", "higher mean count"):
            assert text in r.stdout, text


@pytest.mark.parametrize("extra, what", [
    (("--tip-nodes", "5"), "--tip-nodes"),
    (("--clip-rounds", "3"), "--clip-rounds"),
    (("--drop-isolated",), "--drop-isolated"),
    (("--gfa", "--drop-isolated", "--tip-nodes", "4"), "--clip-tips"),
])
def test_clip_flags_need_clip_tips(cli, tmp_path, extra, what):
    fa, out = tmp_path / "a.fa", tmp_path / "out"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGTAAACCCGGGTTT\n")
    r = run(cli, "unitigs", "-i", fa, "-o", out, "-k", "15", *extra)
    assert r.returncode == 2, r.stderr
    assert r.stderr.startswith("error: ") and what in r.stderr and "--clip-tips" in r.stderr
    assert "For more information, try '--help'." in r.stderr
    assert not out.exists()


@pytest.mark.parametrize("extra, what", [
    (("--clip-tips", "--tip-nodes", "0"), "--tip-nodes"),
    (("--clip-tips", "--tip-nodes", "2147483647"), "--tip-nodes"),
    (("--clip-tips", "--clip-rounds", "0"), "--clip-rounds"),
    (("--clip-tips", "--clip-rounds", "1025"), "--clip-rounds"),
    (("--clip-tips", "yes"), "yes"),
])
def test_clip_flag_values_out_of_range(cli, tmp_path, extra, what):
    fa, out = tmp_path / "a.fa", tmp_path / "out"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGTAAACCCGGGTTT\n")
    r = run(cli, "unitigs", "-i", fa, "-o", out, "-k", "15", *extra)
    assert r.returncode == 2 and r.stderr.startswith("error: ") and what in r.stderr, r.stderr
    assert not out.exists()


def test_the_binding_declares_the_calls():
    from kmertools_amd import _lib, device
    for name in ("erase", "erase_device", "unitig_tips", "unitig_tips_device", "clip_tips"):
        assert callable(getattr(device.Counter, name)), name
    assert (device.TIP_KEEP, device.TIP_TIP, device.TIP_ISOLATED, device.CLIP_ISOLATED) == (0, 1, 2, 1)
    assert device.CLIP_STATS_NAMES == tr.STATS
    for name in ("kt_ctr_erase", "kt_ctr_unitig_tips", "kt_ctr_clip_tips"):
        assert name in _lib.SYMBOLS
    header = (ROOT / "include" / "kmertools_hip.h").read_text()
    for text in ("#define KT_TIP_KEEP 0", "#define KT_TIP_TIP 1", "#define KT_TIP_ISOLATED 2", "#define KT_TIP_TALLY 4",
                 "#define KT_CLIP_ISOLATED 1u", "#define KT_CLIP_STATS 8"):
        assert text in header, text
    assert (_lib.KT_TIP_TALLY, _lib.KT_CLIP_STATS) == (4, 8)


# ---- the reference ----------------------------------------------------------------------------------------------------------

KNOWN = json.loads((ROOT / "tests" / "golden" / "clip_tips_known.json").read_text())["cases"]
LINKS_KNOWN = json.loads((ROOT / "tests" / "golden" / "unitig_links_known.json").read_text())["cases"]


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: c["name"])
def test_reference_reproduces_the_worked_answers(case):
    k, mt = case["k"], case["max_tip_nodes"]
    table = gr.count_strings(case["reads"], k)
    assert [u[0] for u in ur.unitigs(table, k)] == case["unitigs"]
    for drop, pre in ((False, ""), (True, "drop_")):
        red, s, rounds = tr.clip(table, k, mt, drop_isolated=drop)
        assert rounds == case[pre + "rounds"] and s == case[pre + "stats"]
        assert [u[0] for u in ur.unitigs(red, k)] == case[pre + "survivors"]
        assert s[6] == 0 and s[0] == len(rounds) - 1
        assert sum(table.values()) - sum(red.values()) == s[5] and len(table) - len(red) == s[2] + s[4]


def test_the_worked_answers_cover_the_rule():
    by = {c["name"]: c for c in KNOWN}
    # the seven link cases, as they stand in their own file
    for c in LINKS_KNOWN:
        assert by[c["name"]]["reads"] == c["reads"] and by[c["name"]]["k"] == c["k"] and by[c["name"]]["unitigs"] == c["unitigs"]

    def clipped(name, r=0):
        return [u for u, m in zip(by[name]["unitigs"], by[name]["rounds"][r]) if m == tr.TIP]
    assert clipped("Y branch") == ["AATGG"]                    # the weaker branch
    assert clipped("bubble") == ["GCTAAGC"]                    # the dangling end, not the bubble's arms
    assert clipped("palindromic node") == ["CGTCC"]            # a tie on km: the larger number loses
    assert clipped("ends linked to each other") == ["CCTGAA"]
    for name in ("homopolymer", "hairpin", "cycle"):
        assert by[name]["rounds"] == [[0]] and by[name]["drop_rounds"] == [[0]]
    assert clipped("tie at a fork") == ["AATGG"] and by["tie at a fork"]["unitigs"][:2] == ["AATGC", "AATGG"]
    long_tip = by["a tip one node too long"]
    assert not any(long_tip["rounds"][0]) and long_tip["max_tip_nodes"] == 1
    assert tr.clip(gr.count_strings(long_tip["reads"], long_tip["k"]), long_tip["k"], 2)[1][1] > 0  # one node more: it goes
    iso = by["isolated short and long"]
    assert iso["rounds"] == [[0, 2]] and iso["drop_rounds"] == [[0, 2], [0]] and iso["drop_stats"][3:5] == [1, 2]
    cyc = by["tip off a cycle"]
    assert clipped("tip off a cycle") == ["CCTGATGA"] and cyc["survivors"] == ["ATCATCATC"]
    two = by["tip on a tip"]
    assert len(two["rounds"]) == 3 and two["stats"][0] == 2 and sum(two["rounds"][0]) == 1 and sum(two["rounds"][1]) == 1
    assert two["survivors"] == [gr.rc_s("ACGGTCAATGCGTTACAGA")] or two["survivors"] == ["ACGGTCAATGCGTTACAGA"]
    # stopped after one round the call says so, and a second call finishes the job
    table = gr.count_strings(two["reads"], two["k"])
    red, s, _ = tr.clip(table, two["k"], two["max_tip_nodes"], max_rounds=1)
    assert s[0] == 1 and s[6] == 1
    red2, s2, _ = tr.clip(red, two["k"], two["max_tip_nodes"])
    assert s2[0] == 1 and s2[6] == 0 and [u[0] for u in ur.unitigs(red2, two["k"])] == two["survivors"]


def random_reads(rng, k, letters):
    """reads of a small random genome with errors, their reverse complements, a circularised genome (once or several times
    around), homopolymers, repeats of two and four letters and a hairpin appended to a read (as the link tests build them)"""
    L = list(letters)
    g = "".join(rng.choice(L, size=int(rng.integers(k + 2, 50))))
    reads = []
    for _ in range(int(rng.integers(1, 8))):
        a = int(rng.integers(0, len(g) - k))
        s = list(g[a:a + int(rng.integers(k, 3 * k + 4))])
        if rng.random() < 0.4:
            s[int(rng.integers(0, len(s)))] = L[int(rng.integers(0, len(L)))]
        reads.append("".join(s))
        if rng.random() < 0.5:
            reads.append(gr.rc_s(reads[-1]))
    c = "".join(rng.choice(L, size=int(rng.integers(2, 20))))
    reads.append(c * int(rng.integers(1, 4)) + c[:k - 1])
    if rng.random() < 0.5:
        n = k + int(rng.integers(0, 4))
        reads += [L[int(rng.integers(0, len(L)))] * n, ("AT" * n)[:n + 1], ("ACGT" * n)[:n + 2]]
        half = reads[0][:k]
        reads.append(half + gr.rc_s(half))
    return reads


SEEN = dict(tips=0, isolated=0, ties=0, two_rounds=0, tables=0)


@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 7, 9])
def test_the_reference_keeps_its_invariant(k):
    rng = np.random.default_rng(5200 + k)
    for trial in range(24):
        table = gr.count_strings(random_reads(rng, k, "ACGT" if trial % 3 else "AC"), k)
        for lo in (1, 2):
            for mt in (1, k, 2**31 - 2):
                us, ls, m, tally = tr.marks(table, k, mt, lo)  # (asserts the invariant and what a marked unitig is)
                assert len(m) == len(us) and tally[0] + tally[2] == sum(1 for x in m if x)
                if us:  # the array form, on the arrays the library would fill
                    off = np.cumsum([0] + [len(u[0]) for u in us]).astype(np.uint64)
                    loff, lto = lr.as_arrays(ls)
                    m2, t2 = tr.marks_of_arrays(off, np.array([u[1] for u in us], np.uint64), np.array([u[2] for u in us], np.uint32),
                                                loff, lto, k, mt)
                    assert m2.dtype == np.uint8 and m2.tolist() == m and t2.tolist() == tally
                # a tie: two candidates with equal mean counts at one end
                n, c = [u[3] for u in us], [u[1] for u in us]
                cand = [u for u in range(len(us)) if n[u] <= mt and not us[u][2] and bool(ls[2 * u]) != bool(ls[2 * u + 1])]
                for fs in ls:
                    at = [f >> 1 for f in fs if f >> 1 in cand]
                    SEEN["ties"] += any(a != b and c[a] * n[b] == c[b] * n[a] for a in at for b in at)
                SEEN["tips"] += tally[0]
                SEEN["isolated"] += tally[2]
            for drop in (False, True):
                red, s, rounds = tr.clip(table, k, k, 8, drop, lo)
                assert set(red) <= set(table) and all(red[key] == table[key] for key in red)
                assert all(key in red for key in table if table[key] < lo)  # entries that are no nodes are never touched
                assert len(table) - len(red) == s[2] + s[4] and sum(table.values()) - sum(red.values()) == s[5]
                assert s[0] == len(rounds) - (0 if s[6] else 1)
                SEEN["two_rounds"] += s[0] >= 2
            SEEN["tables"] += 1


def test_the_sweep_saw_what_it_is_for():
    assert SEEN["tables"] == 7 * 48, SEEN
    assert SEEN["tips"] and SEEN["isolated"] and SEEN["ties"] and SEEN["two_rounds"], SEEN


def test_clip_stats_rendering():
    assert tr.want_clip_stats([2, 3, 6, 1, 2, 10, 0, 0]) == \
        b"rounds\t2\ntips\t3\ntip_nodes\t6\nisolated\t1\nisolated_nodes\t2\noccurrences\t10\nconverged\t1\n"
    assert tr.want_clip_stats([1, 1, 1, 0, 0, 1, 1, 0]).endswith(b"converged\t0\n")
