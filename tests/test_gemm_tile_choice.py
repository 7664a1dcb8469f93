"""The tile GEMM's tile choice (tile_choice_bf16 / tile_choice_fp8 of ht_vllm_omni_amd/csrc/gemm_tile_policy.h) held to a table, on the CPU.

omni_gemm_tile and omni_gemm_tile_fp8 take the geometry and the kernel form (lock-step <WAVES_N, WN, WM> or two-group MW) of a launch from
those two functions.  Every geometry adds k in the same order, so the choice changes time and never a bit: no GPU test sees it drift; this
one does.

The table (tests/golden/gemm_tile_choice.txt) was NOT produced by the header under test: it was printed by a driver holding verbatim copies
of the dispatch blocks of the two entry points as they stood in the commit before the choice moved into the header (44af730:
gemm_prefill.hip lines 509-547, gemm_prefill_f8.hip lines 448-466), with every launch replaced by a print of its template arguments, over
exactly the cases of `rows()`.  A change of policy changes the table on purpose, in the same commit.

Cases: M in MS; N = every prefill GEMM width of the presets (qkv, o / down, 2 * inter, router, shared expert) plus the Code2Wav and odd
widths of ODD_NS; for the bf16 entry point groups in {1, 5, 128}, plain and windowed (a conv window; the entry point takes a grouped launch
without one only), SiLU-mul on the GU8 row order on and off, and every tile_hint the entry point accepts there (3+ need N % 256 == 0, 5+ a
plain GEMM); for the fp8 entry point, which has neither groups nor windows, GU8 on and off and its hints (1, 3, 4 need N % 256 == 0).
A table entry is "<WAVES_N><WN><WM>" for the lock-step kernel or "P<MW>" for the two-group one."""
import os
import shutil
import subprocess

import pytest

from ht_vllm_omni_amd.config import PRESETS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "ht_vllm_omni_amd", "csrc", "gemm_tile_policy.h")
TABLE = os.path.join(ROOT, "tests", "golden", "gemm_tile_choice.txt")
GXX = shutil.which("g++")

MS = (1, 16, 64, 65, 192, 193, 224, 225, 256, 257, 300, 513, 1000, 3000, 6144, 6400, 6438, 24577)
ODD_NS = (16, 48, 64, 96, 128, 192, 272, 384, 768, 1536)

# the entry points' own step from their arguments to the policy's: `plain` is omni_gemm_tile's condition for the two-group form
MAIN = r"""
#include <cstdio>
#include "%s"
int main() {
    int f8, M, N, groups, windowed, gu8, hint;
    while (std::scanf("%%d %%d %%d %%d %%d %%d %%d", &f8, &M, &N, &groups, &windowed, &gu8, &hint) == 7) {
        const bool plain = groups == 1 && !windowed;
        const TileChoice t = f8 ? tile_choice_fp8(M, N, hint) : tile_choice_bf16(M, N, groups, plain, gu8 != 0, hint);
        if (t.mw) std::printf("P%%d\n", t.mw);
        else std::printf("%%d%%d%%d\n", t.waves_n, t.wn, t.wm);
    }
    return 0;
}
"""


def widths():
    out = set(ODD_NS)
    for d in PRESETS.values():
        out |= {d.qkv_out, d.hidden, 2 * d.inter}
        if d.moe_experts:
            out |= {d.moe_experts, 2 * d.moe_shared_inter}
    return sorted(n for n in out if n % 16 == 0)


def rows():
    """(key, [input line per M]) in table order"""
    out = []
    for n in widths():
        for groups, windowed in ((1, 0), (1, 1), (5, 0), (128, 0)):
            for gu8 in (0, 1):
                for hint in range(8):
                    if (hint >= 3 and n % 256) or (hint >= 5 and (groups > 1 or windowed)):
                        continue
                    out.append(("bf16 N=%d groups=%d windowed=%d gu8=%d hint=%d" % (n, groups, windowed, gu8, hint),
                                ["0 %d %d %d %d %d %d" % (m, n, groups, windowed, gu8, hint) for m in MS]))
    for n in widths():
        for gu8 in (0, 1):
            for hint in range(5):
                if hint in (1, 3, 4) and n % 256:
                    continue
                out.append(("fp8 N=%d gu8=%d hint=%d" % (n, gu8, hint), ["1 %d %d 1 0 %d %d" % (m, n, gu8, hint) for m in MS]))
    return out


def run(exe):
    rs = rows()
    got = subprocess.run([exe], input="\n".join(l for _, ls in rs for l in ls) + "\n", capture_output=True, text=True, check=True).stdout.split()
    table, at = {}, 0
    for key, ls in rs:
        table[key] = " ".join(got[at:at + len(ls)])
        at += len(ls)
    assert at == len(got)
    return table


@pytest.mark.skipif(GXX is None, reason="no g++")
def test_tile_choice_matches_the_table(tmp_path):
    src = tmp_path / "choice_main.cpp"
    src.write_text(MAIN % HEADER.replace("\\", "/"))
    exe = tmp_path / "choice_main"
    subprocess.check_call([GXX, "-std=c++17", "-Wall", "-Werror", str(src), "-o", str(exe)])      # (no HIP: the header is plain host C++)
    got = run(str(exe))
    expected = dict(line.rstrip("\n").split(": ") for line in open(TABLE))
    assert sorted(got) == sorted(expected), "the case list and the table differ: %s" % sorted(set(got) ^ set(expected))[:4]
    bad = {k: (got[k], expected[k]) for k in got if got[k] != expected[k]}
    assert not bad, "%d rows differ (one entry per M; got, expected), e.g. %s" % (len(bad), list(bad.items())[:3])
