"""The decisions of the restarts' agreement (csrc/agree_plan.h) alone: plain host arithmetic, compiled with g++ under
AddressSanitizer + UBSan into a program of its own and run as a program (nothing is loaded into Python)."""
import importlib.util
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Tables: `world` ranks of R restarts; a restart's checksum words are (7, 9) unless a case changes them.  Every case is
# decided once per rank, each from its own copy of the table (what the all-gather hands every rank).
# The emulated agreement: world = 3 x R = 2 label arrays of 37 x 37 entries with 2 .. 7 classes and ~1/3 zeros; the keys by the
# header's arithmetic per rank, summed with wrap-around, relabelled by first occurrence (0 stays 0) -- against refine!
# (src/partitions.jl:62-66: pair code, relabel by first occurrence, 0 only where both are 0) folded over the six.
SRC = r'''
#include <cstdio>
#include <map>
#include <utility>
#include <vector>
#include "agree_plan.h"
using namespace sdpsr;
static unsigned long long state = 777;
static unsigned rnd(unsigned m) { state = state * 6364136223846793005ULL + 1442695040888963407ULL; return (unsigned)((state >> 33) % m); }
static const char* NAMES[] = {"mismatch", "none_valid", "agreed", "meet"};

static std::vector<AgreeRecord> table(int world, int R) {
    std::vector<AgreeRecord> t(world);
    for (auto& r : t) {
        r.len = 1369; r.R = R; r.width = 16;
        for (int i = 0; i < R; ++i) { r.valid[i] = 1; r.word0[i] = 7; r.word1[i] = 9; }
    }
    return t;
}
static void decide(const char* what, int world, int R, const std::vector<AgreeRecord>& t) {
    const AgreePlan p0 = agree_plan(world, t.data());
    bool same = true;
    for (int r = 0; r < world; ++r) {  // every rank decides from its own copy
        std::vector<AgreeRecord> copy(t);
        same = same && agree_plan(world, copy.data()) == p0;
    }
    printf("plan %s world=%d R=%d verdict=%s same=%d\n", what, world, R, NAMES[p0], (int)same);
}
static std::vector<uint32_t> relabel(const std::vector<uint64_t>& key, int* dim) {  // first occurrence, 0 stays 0
    std::map<uint64_t, uint32_t> seen;
    std::vector<uint32_t> out(key.size());
    uint32_t d = 0;
    for (size_t e = 0; e < key.size(); ++e) {
        if (key[e] == 0) { out[e] = 0; continue; }
        auto it = seen.find(key[e]);
        if (it == seen.end()) it = seen.emplace(key[e], ++d).first;
        out[e] = it->second;
    }
    *dim = (int)d;
    return out;
}
static std::vector<uint32_t> refine(const std::vector<uint32_t>& p, const std::vector<uint32_t>& q, int* dim) {
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> seen;
    std::vector<uint32_t> out(p.size());
    uint32_t d = 0;
    for (size_t e = 0; e < p.size(); ++e) {
        if (p[e] == 0 && q[e] == 0) { out[e] = 0; continue; }
        const auto k = std::make_pair(p[e], q[e]);
        auto it = seen.find(k);
        if (it == seen.end()) it = seen.emplace(k, ++d).first;
        out[e] = it->second;
    }
    *dim = (int)d;
    return out;
}
int main() {
    for (int k = 0; k < 200; ++k) printf("m %d %llu\n", k, (unsigned long long)agree_multiplier((uint64_t)k));
    const int worlds[] = {1, 2, 3, 9}, Rs[] = {1, 2, 5};
    for (int world : worlds)
        for (int R : Rs) {
            auto t = table(world, R);
            decide("equal", world, R, t);
            t = table(world, R); t[world - 1].word1[R - 1] ^= 1; decide("word_differs", world, R, t);
            t = table(world, R); t[world / 2].valid[R / 2] = 0; decide("one_invalid", world, R, t);
            t = table(world, R); t[world / 2].valid[R / 2] = 0; t[world / 2].word0[R / 2] = 12345; decide("one_invalid_garbage", world, R, t);
            t = table(world, R); for (auto& r : t) for (int i = 0; i < R; ++i) r.valid[i] = 0; decide("none_valid", world, R, t);
            if (world > 1) {
                t = table(world, R); t[world - 1].len += 1; decide("len_mismatch", world, R, t);
                t = table(world, R); t[1].R = R + 1; decide("R_mismatch", world, R, t);
                t = table(world, R); t[world - 1].width = 32; decide("width_mismatch", world, R, t);
            }
        }
    { auto t = table(1, 1); t[0].R = 65; decide("R_too_large", 1, 65, t); t[0].R = 0; decide("R_zero", 1, 0, t); }
    // the first valid restart is not the first restart: the comparison starts at it
    { auto t = table(2, 2); t[0].valid[0] = 0; t[0].word0[0] = 1; t[1].word0[1] = 8; decide("first_invalid_other_differs", 2, 2, t); }

    const int world = 3, R = 2, len = 37 * 37;
    std::vector<std::vector<uint32_t>> lab(world * R, std::vector<uint32_t>(len));
    for (int s = 0; s < world * R; ++s) {
        const unsigned classes = 2 + (unsigned)s;
        for (int e = 0; e < len; ++e) lab[s][e] = (e % 41 == 0 || rnd(3) == 0) ? 0u : 1u + rnd(classes);  // (every 41st entry: 0 in all six)
        int d; lab[s] = relabel(std::vector<uint64_t>(lab[s].begin(), lab[s].end()), &d);  // canonical, like a restart's result
    }
    std::vector<uint64_t> sum(len, 0);
    for (int rank = 0; rank < world; ++rank) {
        std::vector<uint64_t> keys(len, 0);  // one rank's key pass
        for (int i = 0; i < R; ++i)
            for (int e = 0; e < len; ++e) keys[e] += (uint64_t)lab[rank * R + i][e] * agree_multiplier((uint64_t)(agree_first_slot(rank, R) + i));
        for (int e = 0; e < len; ++e) sum[e] += keys[e];  // the all-reduce
    }
    int dim_keys = 0, dim_fold = 0;
    const std::vector<uint32_t> met = relabel(sum, &dim_keys);
    std::vector<uint32_t> fold = lab[0];
    for (int s = 1; s < world * R; ++s) fold = refine(fold, lab[s], &dim_fold);
    int zeros = 0, zeros_ok = 1;
    for (int e = 0; e < len; ++e) {
        bool allz = true;
        for (int s = 0; s < world * R; ++s) allz = allz && lab[s][e] == 0;
        zeros += allz;
        if (allz != (met[e] == 0)) zeros_ok = 0;
    }
    printf("emulated equal=%d dim_keys=%d dim_fold=%d zeros=%d zeros_ok=%d\n", (int)(met == fold), dim_keys, dim_fold, zeros, zeros_ok);

    const int32_t s1[] = {0}, s2[] = {3}, s3[] = {2, 3, 0, 0}, s4[] = {9, 2, 3}, s5[] = {0, 0, 0};
    printf("winner %d %d %d %d %d\n", agree_winner(1, s1), agree_winner(1, s2), agree_winner(4, s3), agree_winner(3, s4), agree_winner(3, s5));
    printf("first_slot %lld %lld %lld\n", (long long)agree_first_slot(0, 5), (long long)agree_first_slot(3, 5), (long long)agree_first_slot(8, 64));
    return 0;
}
'''


def _run():
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.cpp"), "w") as f:
            f.write(SRC)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                               os.path.join(ROOT, "sdpsymmetryreduction.jl_amd", "csrc"), os.path.join(d, "t.cpp"), "-o", os.path.join(d, "t")])
        return subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, text=True).stdout.splitlines()


def _parallel():
    spec = importlib.util.spec_from_file_location("sdpsr_parallel_for_test", os.path.join(ROOT, "sdpsymmetryreduction.jl_amd", "parallel.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_agree_plan_decisions_multipliers_and_an_emulated_agreement():
    """agree_plan.h under ASan + UBSan: m(k), k < 200, equals parallel._slot_multiplier mod 2^64; the verdicts on hand-made
    tables for world 1, 2, 3, 9 x R = 1, 2, 5, the same from every rank's copy; three ranks of two restarts on 37 x 37 labels
    agree, through per-rank keys and their wrapping sum, on exactly the folded pairwise refinement; the winner rule."""
    out = _run()
    par = _parallel()
    ms = [line.split() for line in out if line.startswith("m ")]
    assert [int(k) for _, k, _ in ms] == list(range(200))
    for _, k, v in ms:
        assert int(v) == par._slot_multiplier(int(k)) % 2 ** 64, k
        assert int(v) % 2 == 1  # odd: injective in the label
    plans = [dict(kv.split("=") for kv in line.split()[2:]) | {"case": line.split()[1]} for line in out if line.startswith("plan ")]
    expect = {"equal": "agreed", "word_differs": "meet", "one_invalid": "meet", "one_invalid_garbage": "meet", "none_valid": "none_valid",
              "len_mismatch": "mismatch", "R_mismatch": "mismatch", "width_mismatch": "mismatch", "R_too_large": "mismatch",
              "R_zero": "mismatch", "first_invalid_other_differs": "meet"}
    seen = set()
    for p in plans:
        want = expect[p["case"]]
        if int(p["world"]) * int(p["R"]) == 1:  # a single restart has nothing to differ from, and without it none is valid
            want = {"word_differs": "agreed", "one_invalid": "none_valid", "one_invalid_garbage": "none_valid"}.get(p["case"], want)
        assert p["verdict"] == want and p["same"] == "1", p
        seen.add((p["case"], int(p["world"]), int(p["R"])))
    for world in (1, 2, 3, 9):
        for R in (1, 2, 5):
            for case in ("equal", "word_differs", "one_invalid", "one_invalid_garbage", "none_valid"):
                assert (case, world, R) in seen
            for case in ("len_mismatch", "R_mismatch", "width_mismatch"):
                assert ((case, world, R) in seen) == (world > 1)
    emu = [dict(kv.split("=") for kv in line.split()[1:]) for line in out if line.startswith("emulated ")]
    assert len(emu) == 1 and emu[0]["equal"] == "1" and emu[0]["zeros_ok"] == "1", emu
    # the case is not trivial: the six arrays really refine each other, and some entries are 0 in all of them
    assert emu[0]["dim_keys"] == emu[0]["dim_fold"] and 100 < int(emu[0]["dim_keys"]) <= 1369 and int(emu[0]["zeros"]) >= 1, emu
    assert out[-2] == "winner 0 -1 2 -1 0"
    assert out[-1] == "first_slot 0 15 512"


def test_agreement_entry_points_are_declared_and_exported(pkg):
    """The new entry points are in include/sdpsr.h and in the library, the binding knows their signatures, the ABI version is
    still 5, and the product library does not link against RCCL (it is opened by SONAME on first use)."""
    names = ["sdpsr_meet_keys", "sdpsr_agree_partitions", "sdpsr_agree_block_diagonalization", "sdpsr_comm_unique_id",
             "sdpsr_comm_create", "sdpsr_comm_rank", "sdpsr_comm_world", "sdpsr_comm_broadcast", "sdpsr_comm_destroy"]
    declared = pkg._lib.declared_symbols()
    lib = pkg.load_library()
    for s in names:
        assert s in declared, s
        assert hasattr(lib, s) and getattr(lib, s).argtypes is not None, s
    assert lib.sdpsr_version() == 5
    assert lib.sdpsr_comm_rank(None) == -1 and lib.sdpsr_comm_world(None) == -1  # (no RCCL needed for these)
    needed = subprocess.run(["readelf", "-d", pkg._lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "NEEDED" in needed and "rccl" not in needed.lower() and "nccl" not in needed.lower()
    for f in (pkg.Comm, pkg.meet_keys, pkg.agree_partitions, pkg.agree_block_diagonalization):
        assert callable(f)
