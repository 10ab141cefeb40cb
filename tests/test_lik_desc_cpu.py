"""The one list of likelihood kinds, the one descriptor check and the facts derived from them (csrc/agpl_lik_desc.h).  The header has
no HIP dependency, so it is compiled here with g++ into a program of its own that prints code and message of agpl_lik_desc_check for
a grid of descriptors; the table below states what every entry point answered before the check was shared (the message strings are
those of the extension libraries' copies, character for character).  The sources are read as well: the five files that used to carry
a copy call the shared check and state no parameter rule or bound on the kind of their own, and the list names every enumerator of
include/agpl.h exactly once."""
import math
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
SITES = ("agpl_core.hip", "agpl_predictive.hip", "agpl_likgrad.hip", "agpl_quantile.hip", "agpl_sample_y.hip")

OK, INVALID = 0, -1
NAN, INF = float("nan"), float("inf")
M_KIND = "unknown likelihood kind %d"
M_NLATENT = "nlatent = %d, expected %d"
M_CAT = "categorical needs 1 <= nlatent <= 64 and logtheta"
M_R = "NegBinomial failures r must be > 0"
M_N = "Binomial trials n must be an integer with 1 <= n < 4194304 = 2^22 (n = %g)"
M_T = "StudentT needs nu > 0 and sigma > 0"
M_LAMBDA = "the link's scale lambda must be > 0"
M_BETA = "Laplace needs beta > 0"
M_ALD = "AsymmetricLaplace needs a finite sigma > 0 and 0 < tau < 1 (sigma = %g, tau = %g)"
M_LOGISTIC = "LogisticNoise needs a finite scale > 0 (scale = %g)"
PARAMETER_MESSAGES = (M_R, M_N.split(" (")[0], M_T, M_LAMBDA, M_BETA, "AsymmetricLaplace needs", "LogisticNoise needs")

# (kind, nlatent, p0, p1, logtheta given, code, message)
CASES = [
    # one valid descriptor per kind (the ends of the Binomial's and the categorical kinds' ranges included)
    (0, 1, 0.0, 0.0, False, OK, ""),
    (1, 1, 2.5, 0.0, False, OK, ""),
    (2, 1, 3.0, 1.5, False, OK, ""),
    (3, 3, 0.0, 0.0, True, OK, ""),
    (3, 1, 0.0, 0.0, True, OK, ""),
    (3, 64, 0.0, 0.0, True, OK, ""),
    (4, 2, 0.0, 0.0, True, OK, ""),
    (4, 64, 0.0, 0.0, True, OK, ""),
    (5, 1, 4.0, 0.0, False, OK, ""),
    (6, 1, 0.7, 0.0, False, OK, ""),
    (7, 2, 2.0, 0.0, False, OK, ""),
    (8, 1, 1.0, 0.0, False, OK, ""),
    (8, 1, 4194303.0, 0.0, False, OK, ""),
    (9, 1, 0.5, 0.25, False, OK, ""),
    (10, 1, 0.7, 0.0, False, OK, ""),
    (11, 1, 0.0, 0.0, False, OK, ""),
    (11, 1, -3.0, NAN, False, OK, ""),  # (p[] of the per-point Binomial is not read)
    # unknown kinds
    (-1, 1, 0.0, 0.0, False, INVALID, M_KIND % -1),
    (12, 1, 0.0, 0.0, False, INVALID, M_KIND % 12),
    # nlatent
    (0, 0, 0.0, 0.0, False, INVALID, M_NLATENT % (0, 1)),
    (0, 2, 0.0, 0.0, False, INVALID, M_NLATENT % (2, 1)),
    (6, 2, 0.7, 0.0, False, INVALID, M_NLATENT % (2, 1)),
    (11, 2, 0.0, 0.0, False, INVALID, M_NLATENT % (2, 1)),
    (7, 1, 2.0, 0.0, False, INVALID, M_NLATENT % (1, 2)),
    (3, 0, 0.0, 0.0, True, INVALID, M_CAT),
    (3, 65, 0.0, 0.0, True, INVALID, M_CAT),
    (3, 3, 0.0, 0.0, False, INVALID, M_CAT),
    (4, 0, 0.0, 0.0, True, INVALID, M_CAT),
    (4, 65, 0.0, 0.0, True, INVALID, M_CAT),
    (4, 2, 0.0, 0.0, False, INVALID, M_CAT),
]
CASES += [(1, 1, r, 0.0, False, INVALID, M_R) for r in (0.0, -1.0, NAN, INF)]
CASES += [(8, 1, n, 0.0, False, INVALID, M_N % n) for n in (0.0, 0.5, 1.5, 4194304.0, NAN)]
CASES += [(2, 1, nu, sg, False, INVALID, M_T) for nu, sg in ((0.0, 1.0), (-1.0, 1.0), (3.0, 0.0), (INF, 1.0), (3.0, INF), (NAN, 1.0))]
CASES += [(kind, nl, lam, 0.0, False, INVALID, M_LAMBDA) for kind, nl in ((5, 1), (7, 2)) for lam in (0.0, -1.0, NAN, INF)]
CASES += [(6, 1, beta, 0.0, False, INVALID, M_BETA) for beta in (0.0, -1.0, NAN, INF)]
CASES += [(9, 1, sg, 0.5, False, INVALID, M_ALD % (sg, 0.5)) for sg in (0.0, INF, NAN)]
CASES += [(9, 1, 0.5, tau, False, INVALID, M_ALD % (0.5, tau)) for tau in (0.0, 1.0, NAN)]
CASES += [(10, 1, s, 0.0, False, INVALID, M_LOGISTIC % s) for s in (0.0, -1.0, INF, NAN)]

SRC = r"""
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "agpl_lik_desc.h"
static const double logtheta[65] = {0};
static void show(const agpl_lik_desc *d) {
    char err[512];
    strcpy(err, "");
    const int32_t rc = agpl_lik_desc_check(d, err, sizeof(err));
    printf("%d|%s\n", rc, err);
}
static void one(int kind, int nlatent, double p0, double p1, int given) {
    const agpl_lik_desc d = {kind, nlatent, {p0, p1, 0.0, 0.0}, given ? logtheta : nullptr};
    show(&d);
}
// the facts that sites used to restate, at compile time
static_assert(agpl_lik_kind_known(AGPL_LIK_BERNOULLI_LOGISTIC) && agpl_lik_kind_known(AGPL_LIK_BINOMIAL_N), "the ends of the list");
static_assert(!agpl_lik_kind_known(-1) && !agpl_lik_kind_known(12), "beyond the list");
static_assert(lik_is_categorical(AGPL_LIK_CATEGORICAL) && lik_is_categorical(AGPL_LIK_CATEGORICAL_BIJ) && !lik_is_categorical(AGPL_LIK_POISSON), "");
static_assert(agpl_lik_nlatent(AGPL_LIK_HETEROGAUSS) == 2 && agpl_lik_nlatent(AGPL_LIK_LAPLACE) == 1, "");
static_assert(agpl_lik_nparams(AGPL_LIK_BERNOULLI_LOGISTIC) == 0 && agpl_lik_nparams(AGPL_LIK_BINOMIAL) == 0 &&
              agpl_lik_nparams(AGPL_LIK_BINOMIAL_N) == 0 && agpl_lik_nparams(AGPL_LIK_STUDENTT) == 2 &&
              agpl_lik_nparams(AGPL_LIK_NEGBINOMIAL) == 1 && agpl_lik_nparams(AGPL_LIK_POISSON) == 1 && agpl_lik_nparams(AGPL_LIK_LAPLACE) == 1 &&
              agpl_lik_nparams(AGPL_LIK_HETEROGAUSS) == 1 && agpl_lik_nparams(AGPL_LIK_ASYMLAPLACE) == 1 &&
              agpl_lik_nparams(AGPL_LIK_LOGISTIC_NOISE) == 1, "include/agpl_likgrad.h");
int main() {
    show(nullptr);
    // a refusal without a buffer is still a refusal
    printf("%d\n", agpl_lik_desc_check(nullptr, nullptr, 0));
    // the host switch: the body runs for the matching kind alone and its answer comes back; no kind of the list, no call
    for (int kind = -1; kind <= 12; ++kind) {
        int seen = -100, calls = 0;
        const bool got = agpl::lik_switch(kind, [&](auto K) {
            seen = K();
            ++calls;
            return K() != AGPL_LIK_STUDENTT;
        });
        printf("switch %d %d %d %d\n", kind, seen, calls, (int)got);
    }
CASES
    return 0;
}
"""


def _c(x):
    return "NAN" if math.isnan(x) else ("INFINITY" if x > 0 else "-INFINITY") if math.isinf(x) else repr(x)


def _run(tmp_path, extra=()):
    calls = "\n".join("    one(%d, %d, %s, %s, %d);" % (k, nl, _c(p0), _c(p1), lt) for k, nl, p0, p1, lt, _, _ in CASES)
    src = tmp_path / "lik_desc.cpp"
    src.write_text(SRC.replace("CASES", calls))
    exe = tmp_path / "lik_desc"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *extra, "-I", CSRC, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def test_code_and_message_over_the_grid(tmp_path):
    lines = _run(tmp_path)
    assert lines[0] == "-1|null likelihood descriptor" and lines[1] == "-1"
    for kind, ln in zip(range(-1, 13), lines[2:16]):
        known = 0 <= kind <= 11
        assert ln == "switch %d %d %d %d" % (kind, kind if known else -100, known, known and kind != 2), ln
    got = lines[16:]
    assert len(got) == len(CASES)
    for case, ln in zip(CASES, got):
        assert ln == "%d|%s" % (case[5], case[6]), (case, ln)


def test_the_grid_covers_what_it_names():
    valid = {c[0] for c in CASES if c[5] == OK}
    assert valid == set(range(12))
    assert {c[2] for c in CASES if c[0] == 8 and c[5] == OK} == {1.0, 4194303.0}
    refused = [c for c in CASES if c[5] == INVALID]
    assert len(refused) == 13 + 4 + 5 + 6 + 8 + 4 + 6 + 4
    assert all(c[6] for c in refused)


def _read(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as fh:
        return fh.read()


def test_the_five_sites_call_the_shared_check_and_state_none_of_it():
    for name in SITES:
        src = _read(name)
        assert src.count("AGPL_LIK_CHECK(ctx, lik);") == 1, name
        for msg in PARAMETER_MESSAGES + ("unknown likelihood kind", "null likelihood descriptor", "categorical needs", "nlatent = %d"):
            assert msg not in src, (name, msg)
        assert not re.search(r"kind\s*[<>]=?\s*AGPL_LIK_", src), name
        assert "agpl_asymlaplace_ok(" not in src and "agpl_logistic_noise_ok(" not in src, name
        assert "lik->kind == AGPL_LIK_HETEROGAUSS ? 2 : 1" not in src and "want_l" not in src, name
    common = _read("agpl_common.h")
    assert '#include "agpl_lik_desc.h"' in common and common.count("#define AGPL_LIK_CHECK(ctx, lik)") == 1
    assert "agpl_lik_desc_check((lik)" in common
    # every message is stated in the header, once
    desc = _read("agpl_lik_desc.h")
    for msg in PARAMETER_MESSAGES + ("unknown likelihood kind %d", "null likelihood descriptor", M_CAT, M_NLATENT):
        assert desc.count(msg) == 1, msg
    for msg in PARAMETER_MESSAGES + ("unknown likelihood kind", M_CAT):  # ... and nowhere else in csrc/
        for other in os.listdir(CSRC):
            if other != "agpl_lik_desc.h" and other.endswith((".h", ".hip")):
                assert msg not in _read(other), (other, msg)


def test_the_list_names_every_enumerator_once_and_both_switches_expand_it():
    h = open(os.path.join(ROOT, "include", "agpl.h"), encoding="utf-8").read()
    enum = h[h.index("typedef enum {\n    AGPL_LIK_BERNOULLI_LOGISTIC"):h.index("} agpl_lik_kind;")]
    names = re.findall(r"^\s*(AGPL_LIK_\w+)\s*=\s*(\d+)", enum, flags=re.M)
    assert [int(v) for _, v in names] == list(range(12))
    desc = _read("agpl_lik_desc.h")
    body = re.search(r"#define AGPL_LIK_KINDS\(X\)((?:[^\n]*\\\n)+[^\n]*)\n", desc).group(1)
    assert re.findall(r"X\((\w+)\)", body) == [n for n, _ in names]  # each once, in enumerator order
    assert desc.count("AGPL_LIK_KINDS(AGPL_LIK_CASE_)") == 1 and "inline bool lik_switch(int kind, BODY body)" in desc
    rules = _read("agpl_lik_rules.h")
    dispatch = rules[rules.index("void lik_dispatch("):rules.index("ald_beta")]
    assert "AGPL_LIK_KINDS(AGPL_LIK_CASE_)" in dispatch and "AGPL_LIK_CASE_(AGPL_LIK_" not in rules
    assert "lik_is_categorical(int kind)" in desc and "lik_is_categorical(int kind)" not in rules
    # no launch site keeps a list of cases of its own, or a default that stands for a kind
    for name in SITES[1:] + ("agpl_sampler.hip", "agpl_operators.hip"):
        src = _read(name)
        assert "lik_switch(" in src and not re.search(r"case AGPL_LIK_\w+:\s*AGPL_LAUNCH_", src), name
        assert not re.search(r"default:\s*AGPL_LAUNCH_", src) and not re.search(r"#define AGPL_LAUNCH_(PRED|ELL|CDF|QT|SY|AUX|GIBBS_S)\b", src), name
    # the number of learnable parameters is read from the header by both places of agpl_likgrad.hip
    lg = _read("agpl_likgrad.hip")
    assert lg.count("agpl_lik_nparams(") == 2 and "NParams" not in lg
