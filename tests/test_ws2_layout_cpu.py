"""The map of the context's small workspace (csrc/agpl_ws2.h).  The header has no HIP dependency, so it is compiled here with g++: its
static assertions on the fixed head (regions pairwise disjoint, the zero-between-launches words in one range, all inside the head) are
part of the program, and main() checks every tail layout -- the update with S, the factor form, the draw with and without padding, the
dense step -- on both routes for every (M, L) below: every region 256-byte aligned, at or beyond the head, inside `total`, pairwise
disjoint, as large as what its user writes there (stated here independently of the header: L M^2 doubles at the M the factor kernels
run on, L M doubles for a vector, one info word per latent from the hand-written kernels and two from the library), and the layout a
function of its arguments only.  The bytes of the factor kernels' own work area are an argument of the layouts; a stand-in is used."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = r"""
#include <stdio.h>
#include <string.h>
#include <vector>
#include "agpl_ws2.h"
struct Region { const char *name; size_t off, need; };
static int check(const char *what, int M, int L, int route, const std::vector<Region> &r, size_t total) {
    for (size_t i = 0; i < r.size(); ++i) {
        int rc = 0;
        if (r[i].off % 256) rc = 1;
        else if (r[i].off < agpl::kWs2Head) rc = 2;
        else if (r[i].off + r[i].need > total) rc = 3;
        for (size_t j = 0; j < i && !rc; ++j)
            if (r[i].need && r[j].need && r[i].off < r[j].off + r[j].need && r[j].off < r[i].off + r[i].need) rc = 4;
        if (rc) { printf("FAIL %s M=%d L=%d route=%d region %s rc=%d\n", what, M, L, route, r[i].name, rc); return 1; }
    }
    return 0;
}
static int pad_expected(int M) { return M <= 512 ? (M + 31) / 32 * 32 : (M <= 2048 ? (M + 127) / 128 * 128 : M); }
int main() {
    const int Ms[] = {1, 32, 37, 200, 512, 544, 1024, 1100, 1280, 2048, 2176, 600, 1300};
    const int Ls[] = {1, 2, 8, 9, 40, 64};
    if (agpl_factor_pad_m(37) != 64 || agpl_factor_pad_m(200) != 224 || agpl_factor_pad_m(600) != 640 || agpl_factor_pad_m(1300) != 1408) {
        printf("FAIL pad\n");
        return 1;
    }
    long cases = 0;
    for (int M : Ms)
        for (int L : Ls) {
            const size_t mat = 8 * (size_t)L * M * M, work = 8 * (size_t)L * (3 * (size_t)M * M + M) + 1000; // (a stand-in, not a multiple of 256)
            const bool takes = M % 32 == 0 && (M <= 512 || (M <= 2048 && M % 128 == 0)); // L <= 64 throughout
            if (agpl_factor_takes(M, L) != takes || agpl_factor_takes(M, 65)) { printf("FAIL takes M=%d L=%d\n", M, L); return 1; }
            for (int hand = 0; hand <= (takes ? 1 : 0); ++hand) {
                const size_t info = hand ? 4 * (size_t)L : 8 * (size_t)L, hm = hand ? mat : 0, hw = hand ? work : 0;
                for (int own = 0; own <= 1; ++own, ++cases) {
                    const agpl_ws2_update_layout a = agpl_ws2_update(M, L, hand, own, work), b = agpl_ws2_update(M, L, hand, own, work);
                    if (memcmp(&a, &b, sizeof(a))) { printf("FAIL update repeat\n"); return 1; }
                    if (check("update", M, L, 2 * hand + own, {{"info", a.info, info}, {"T", a.T, hm}, {"A", a.A, hm}, {"Uz", a.Uz, hm},
                                                              {"S", a.S, own ? mat : 0}, {"work", a.work, hw}}, a.total)) return 1;
                }
                const agpl_ws2_factor_layout a = agpl_ws2_factor(M, L, hand, work), b = agpl_ws2_factor(M, L, hand, work);
                if (memcmp(&a, &b, sizeof(a))) { printf("FAIL factor repeat\n"); return 1; }
                if (check("factor", M, L, hand, {{"info", a.info, info}, {"T", a.T, hm}, {"work", a.work, hw}}, a.total)) return 1;
                ++cases;
            }
            // the draw chooses its own route: the hand-written kernels at the padded count, the library at M
            const int Mf = pad_expected(M);
            const bool dh = Mf <= 2048, padded = dh && Mf != M;
            const int Mw = dh ? Mf : M;
            const size_t dmat = 8 * (size_t)L * Mw * Mw, dvec = 8 * (size_t)L * Mw;
            const agpl_ws2_draw_layout d = agpl_ws2_draw(M, L, work), e = agpl_ws2_draw(M, L, work);
            if (d.Mf != Mf || d.hand != dh || d.Mf != e.Mf || d.hand != e.hand || d.info != e.info || d.T != e.T || d.A != e.A ||
                d.vf != e.vf || d.z != e.z || d.work != e.work || d.Gp != e.Gp || d.gp != e.gp || d.ep != e.ep || d.total != e.total) {
                printf("FAIL draw M=%d L=%d: Mf %d hand %d\n", M, L, d.Mf, (int)d.hand);
                return 1;
            }
            if (check("draw", M, L, dh, {{"info", d.info, dh ? 4 * (size_t)L : 8 * (size_t)L}, {"T", d.T, dh ? dmat : 0}, {"A", d.A, dmat},
                                        {"vf", d.vf, dvec}, {"z", d.z, dvec}, {"work", d.work, dh ? work : 0},
                                        {"Gp", d.Gp, padded ? dmat : 0}, {"gp", d.gp, padded ? dvec : 0}, {"ep", d.ep, padded ? dvec : 0}},
                      d.total)) return 1;
            ++cases;
        }
    const agpl_ws2_dense_layout n = agpl_ws2_dense(), n2 = agpl_ws2_dense();
    if (memcmp(&n, &n2, sizeof(n)) || check("dense", 0, 1, 0, {{"info", n.info, 8}, {"Ubuf", n.Ubuf, 8 * 64 * 64}}, n.total)) return 1;
    printf("OK %ld cases; head %zu, %d partials, %d flag words, bad-gamma word %d\n", cases, (size_t)agpl::kWs2Head, agpl::kRedParts,
           agpl::kWs2FlagWords, agpl::kWs2BadGammaWord);
    return 0;
}
"""


def test_ws2_layouts(tmp_path):
    src = tmp_path / "ws2.cpp"
    src.write_text(SRC)
    exe = tmp_path / "ws2"
    inc = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", inc, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK"), out.stdout
    # the numbers the kernels were built with: 1016 partials to the last byte below the queues, 1984 flag words to the head's end
    assert "head 16384, 1016 partials, 1984 flag words, bad-gamma word 8" in out.stdout, out.stdout
