"""Census of the stream-taking entry points (no GPU): every function include/genconvit_hip.h declares with a gcv_stream
parameter is either run through the stream protocol by a case of tests/test_streams_gpu.py (streamutil.COVERED) or listed
with a reason (streamutil.EXEMPT).  A new stream-taking entry point without a case fails here."""
from tests import streamutil as su


def test_the_header_parser_finds_the_stream_parameter():
    text = """
    /* int gcv_in_a_comment(int a, gcv_stream s); */
    int gcv_one(const void* x, int n,
                gcv_stream stream);
    int  gcv_two(gcv_handle* h);   // gcv_stream s
    typedef void* gcv_stream;
    const char* gcv_three(gcv_stream s);
    """
    assert su.stream_entry_points(text) == ["gcv_one", "gcv_three"]


def test_every_stream_taking_entry_point_is_covered_or_exempt_with_a_reason():
    declared = su.stream_entry_points()
    assert len(declared) == len(set(declared)) and len(declared) > 60, "the header parse lost its footing"
    for known in ("gcv_ed_forward", "gcv_genconvit_explain_at", "gcv_sig_link", "gcv_k_fused_mlp_timed", "gcv_allgather_logits"):
        assert known in declared
    both = su.COVERED & set(su.EXEMPT)
    assert not both, f"both covered and exempt: {sorted(both)}"
    missing = [n for n in declared if n not in su.COVERED and n not in su.EXEMPT]
    assert not missing, (f"stream-taking entry points with neither a case in tests/test_streams_gpu.py (streamutil.COVERED) "
                         f"nor an exemption (streamutil.EXEMPT): {missing}")
    stale = sorted((su.COVERED | set(su.EXEMPT)) - set(declared))
    assert not stale, f"listed in streamutil but not declared with a gcv_stream parameter: {stale}"
    for name, reason in su.EXEMPT.items():
        assert isinstance(reason, str) and len(reason.strip()) >= 20 and "\n" not in reason, f"{name}: a one-line reason"


def test_covered_is_what_the_gpu_cases_run():
    from tests import test_streams_gpu as gpu
    ran = {e for entries, _ in gpu.CASES.values() for e in entries}
    assert ran == set(su.COVERED), (f"cases without COVERED: {sorted(ran - su.COVERED)}; COVERED without a case: "
                                    f"{sorted(su.COVERED - ran)}")
    # the parametrisation is the table: one pytest case per entry of CASES
    marks = [m for m in gpu.test_late_inputs_and_an_early_clobber_do_not_change_the_result.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and list(marks[0].args[1]) == list(gpu.CASES)
    for which in gpu.CONTROLS:
        assert "gcv_" + which in su.COVERED
