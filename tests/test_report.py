"""The reporting step's two CPU forms (tests/report_oracle.py) agree: the definition and the
parallel form the kernels of wf_report.hip follow, on every hand-built case (with its stated
record count) and on 3,000 seeded random sets per kind whose small coordinate ranges make most
sets drop something.  Also the binding of the new entries and option, and the flag on both
parsers.  No GPU."""
import ctypes as C
import os
import re

import pytest

import report_cases as rc
import report_oracle as ro
from waafle_amd import lib, search, workflow

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(rc.UNGAPPED))
def test_ungapped_cases_both_forms(name):
    raw, min_score, n = rc.UNGAPPED[name]()
    want = ro.hsps_pairwise(raw, min_score)
    assert want == ro.hsps_reach(raw, min_score)
    assert len(want) == n
    assert len(set(want)) == n


@pytest.mark.parametrize("name", sorted(rc.GAPPED))
def test_gapped_cases_both_forms(name):
    raw, min_score, n, raw_alignments = rc.GAPPED[name]()
    want = ro.alns_greedy(raw, min_score)
    assert want == ro.alns_any(raw, min_score)
    assert (len(want[0]), want[1]) == (n, raw_alignments)


def test_field_extremes_make_every_word_count():
    assert [rc.key_words(rc.u_field_extremes(w)[0], False) for w in (1, 2, 3)] == [1, 2, 3]
    assert [rc.key_words(rc.g_field_extremes(w)[0], True) for w in (1, 2, 3, 4, 5)] == [1, 2, 3, 4, 5]


def test_ungapped_forms_agree_on_random_sets():
    hsps = dropped = 0
    for seed in range(3000):
        raw = rc.random_hsps(5 + seed % 29, seed, 1 + seed % 4, span=12)
        a = ro.hsps_pairwise(raw, 3)
        assert a == ro.hsps_reach(raw, 3), seed
        hsps += len(raw)
        dropped += len(raw) - len(a)
    assert dropped > hsps // 2


def test_gapped_forms_agree_on_random_sets():
    alns = dropped = 0
    for seed in range(3000):
        raw = rc.random_anchors(5 + seed % 37, seed, 1 + seed % 3, span=8)
        a = ro.alns_greedy(raw, 1)
        assert a == ro.alns_any(raw, 1), seed
        alns += len(raw)
        dropped += len(raw) - len(a[0])
    assert dropped > alns // 5


def test_binding_matches_header():
    text = open(os.path.join(REPO, "include", "waafle_hip.h")).read()
    assert re.search(r"WF_OPT_SEARCH_REPORT\s*=\s*6\b", text) and lib.OPT_SEARCH_REPORT == 6
    assert re.search(r"#define WF_ABI_VERSION 6\b", text)
    for struct, cls in (("wf_report_hsps", lib.WfReportHsps), ("wf_report_anchors", lib.WfReportAnchors)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [m.group(1) for m in re.finditer(r"(\w+)\s*;", body)]
        assert names == [f for f, _ in cls._fields_]
        assert C.sizeof(cls) == 16 + 8 * (len(names) - 3)        # n, min_score + _pad, then pointers
    for name in ("wf_search_report", "wf_search_report_gapped"):
        assert re.search(r"^int %s\(wf_ctx\* ctx," % name, text, re.M)
        assert name in lib.SIGNATURES and hasattr(lib.load(), name)
    assert [f for f, _ in search.HSP_FIELDS] == [f for f, _ in lib.WfReportHsps._fields_ if f not in ("n", "min_score", "_pad")]
    assert [f for f, _ in search.ANCHOR_FIELDS] == [f for f, _ in lib.WfReportAnchors._fields_
                                                    if f not in ("n", "min_score", "_pad")]


def test_both_parsers_have_report_on():
    for parser, argv in ((search.build_parser(), ["q.fna", "db.fna"]),
                         (workflow.build_parser(), None)):
        action = {a.dest: a for a in parser._actions}["report_on"]
        assert action.option_strings == ["--report-on"] and action.default == "host"
        assert list(action.choices) == ["host", "device"]
    args = search.build_parser().parse_args(["q.fna", "db.fna", "--report-on", "device"])
    assert args.report_on == "device"
    with pytest.raises(SystemExit):
        search.build_parser().parse_args(["q.fna", "db.fna", "--report-on", "gpu"])
