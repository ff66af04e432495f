"""CPU tests of the table of device entries (tests/stream_cases.py): every exported function with a ``hip_stream`` parameter has
exactly one row, every row names such a function and carries the word its header uses, and no row's poison input gives what its real
input gives - in any output that tests/test_gpu_streams.py compares.  No GPU: the expectations are the host models'."""
from __future__ import annotations

import re

import numpy as np
import pytest

import stream_cases as SC
from conftest import ROOT


def test_every_declared_stream_entry_has_exactly_one_row():
    declared = SC.declared()
    names = [r.function for r in SC.rows()]
    print(f"{len(declared)} declarations with a hip_stream parameter in {len(set(declared.values()))} headers, {len(names)} rows")
    assert set(SC.INTERNAL) <= set(declared) and {r.function for r in SC.extra_rows()} <= set(names)
    assert len(declared) >= 40
    twice = sorted({n for n in names if names.count(n) > 1})
    assert not twice, f"more than one row: {twice}"
    missing = sorted(set(declared) - set(names))
    assert not missing, f"declared with a hip_stream parameter, but without a row in tests/stream_cases.py: {missing}"
    unknown = sorted(set(names) - set(declared))
    assert not unknown, f"rows that name no declared function: {unknown}"


def test_the_parser_sees_a_new_declaration(tmp_path, monkeypatch):
    """The completeness test's own instrument: a header with one more entry is one more name, wherever the parameter stands and however
    the declaration is broken into lines; a comment that mentions hip_stream is none."""
    inc = tmp_path / "include"
    inc.mkdir()
    (inc / "a.h").write_text("/* queued on hip_stream (void *hip_stream); */\nint  mdemod_new_thing_device(const int8_t *x_dev, uint64_t n,\n"
                             "                             int device, void *hip_stream);\nint mdemod_other(void *hip_stream, int x);\nint mdemod_host_only(int device);\n")
    monkeypatch.setattr("conftest.ROOT", tmp_path)
    assert SC.declared() == {"mdemod_new_thing_device": "include/a.h", "mdemod_other": "include/a.h"}


def _comment_before(text: str, name: str) -> str:
    """The comments between the previous declaration's end and ``name`` - and, for the link variant (whose comments refer to the
    plain entries), nothing more."""
    spans = [m.span() for m in re.finditer(r"/\*.*?\*/", text, flags=re.S)]
    at = next(m.start() for m in re.finditer(rf"\b{name}\s*\(", text) if not any(a <= m.start() < b for a, b in spans))
    head = text[:at]
    cut = max(head.rfind(";"), head.rfind("}"))
    # a comment may itself hold a ';': take every comment that ends behind the last declaration's end
    comments = [m for m in re.finditer(r"/\*.*?\*/", head, flags=re.S) if m.end() > cut or m.start() > cut]
    return " ".join(m.group(0) for m in comments)


@pytest.mark.parametrize("row", SC.all_rows(), ids=str)
def test_contract_is_the_headers_word(row):
    """The comment that stands in front of the declaration says "asynchronous" for an ``async`` row, and "synchronous", "waits for" or
    "returns after" for a ``sync`` one - not both, and one of them."""
    assert row.contract in ("async", "sync")
    header = SC.declared()[row.function]
    text = (ROOT / header).read_text()
    comment = _comment_before(text, row.function).lower()
    says_async = bool(re.search(r"\basynchronous\b", comment))
    says_sync = bool(re.search(r"\bsynchronous\b|\bwaits for hip_stream\b|\breturns after its kernels\b", comment))
    if row.function == "mdemod_il_deinterleave_device":                       # "asynchronous for up to 32 segments ..., synchronous for more"
        assert says_async and says_sync
        says_async, says_sync = row.case == "", row.case != ""                # the row of the table has 4 segments, the second case 33
    print(f"{row.function} ({header}): {row.contract}; the comment: async {says_async}, sync {says_sync}")
    assert says_async != says_sync, f"{header}: the comment in front of {row.function} must say whether the call is asynchronous or synchronous"
    assert (row.contract == "async") == says_async


@pytest.mark.parametrize("row", SC.all_rows(), ids=str)
def test_poison_differs_from_real(row):
    real, poison = SC.case(row.key, "real"), SC.case(row.key, "poison")
    assert sorted(real) == sorted(poison)
    for k in real:
        assert real[k].shape == poison[k].shape and real[k].dtype == poison[k].dtype, k       # an input of the same shape
    assert any(not np.array_equal(real[k], poison[k]) for k in real)
    want, other = SC.want(row.key, "real"), SC.want(row.key, "poison")
    assert row.differs(list(want), list(other)), f"{row.function}: an output is the same for the poison as for the real input"
