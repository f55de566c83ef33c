"""-m gpu: refused context calls say what they said.  tests/ctx_refusals.py makes every refused call of its list -- at least one through
each front the context's calls share (offset check, host-batch upload, stream continuation, poisoned refusal, block table, raw range
coder) -- and tests/golden/ctx_refusals.json holds the (return code, leon_last_error text) pairs the library gave when each call still
carried its own copy of that front."""
import json

import pytest

import ctx_refusals

pytestmark = pytest.mark.gpu


def test_refused_context_calls_say_what_they_said():
    want = json.load(open(ctx_refusals.PATH))
    got = ctx_refusals.replay()
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], name
