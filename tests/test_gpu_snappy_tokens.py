"""K1 (Snappy) on the GPU, token by token: the hand-assembled streams of snappy_tokens.py through
GpuDecoder.snappy_decompress. Every valid stream must come out byte for byte as the assembler expects
(test_snappy_tokens.py shows on the CPU that the oracle and pyarrow read it the same way) AND take the
path its case pins: the serial kernel decodes anything, so a test that accepted any
pf_snappy_last_fallback would let the block-parallel path fail silently into it. Codes
(pf_snappy_par.h): 0 block-parallel, 2 pieces re-run as one page, 3 serial kernel.
The four token decoders under test: walk_tok (index pass), snap_tok / tag_tl / tag_ol, snap_tok32
(executor producer) and serial_page's own parse. Invalid streams must be refused with
PF_ERR_CORRUPT_PAGE wherever the oracle refuses them, and leave the decoder usable."""
import pytest

import snappy_tokens as T

pytestmark = pytest.mark.gpu

PF_ERR_CORRUPT_PAGE = -2
GROUPS = "abcdefgh"


@pytest.fixture(scope="module")
def dec():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


def _check(dec, cases, label=""):
    wrong = []
    for name, stream, exp, fb, _tags in cases:
        got, code = dec.snappy_decompress(stream, cap=max(1, len(exp)))
        if got != exp:
            at = next((i for i, (x, y) in enumerate(zip(got, exp)) if x != y), min(len(got), len(exp))) if isinstance(got, bytes) else got
            wrong.append(f"{label}{name}: output differs (first at byte {at} of {len(exp)}; status / code {code})")
        elif code != fb:
            wrong.append(f"{label}{name}: pf_snappy_last_fallback {code}, expected {fb}")
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("group", GROUPS)
def test_valid_streams(dec, group):
    """The default executor (k_snappy_exec5)."""
    _check(dec, T.valid_corpus()[group])


@pytest.mark.parametrize("group", GROUPS)
def test_valid_streams_exec2(switches, group):
    """The diagnostics build's one-wave-per-piece executor (k_snappy_exec2), as test_executors_agree."""
    from pfloor.decoder import GpuDecoder
    with switches(PF_EXEC="2"), GpuDecoder(0) as d:
        _check(d, T.valid_corpus()[group], "PF_EXEC=2 ")


def test_invalid_streams_refused(dec, oracle):
    """Status parity with the oracle on invalid raw streams, at the first token, in the second 64 KiB
    piece and at the last token; the decoder decodes a valid stream right after each."""
    name0, good, exp0, fb0, _ = T.valid_corpus()["g"][0]
    wrong = []
    for i, (name, stream, declared) in enumerate(T.invalid_corpus()):
        r = oracle.snappy_uncompress(stream)
        assert r is None or (isinstance(r, int) and r < 0), name
        rc, out = dec.snappy_decompress(stream, cap=max(1, declared))
        if out is not None or rc != PF_ERR_CORRUPT_PAGE:
            wrong.append(f"{name}: {rc if out is None else 'accepted'}")
        got, code = dec.snappy_decompress(good, cap=len(exp0))
        assert got == exp0 and code == fb0, f"{name0} after {name}"
    assert not wrong, "\n".join(wrong)
