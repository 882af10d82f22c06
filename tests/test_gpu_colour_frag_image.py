"""nrc_ngp_colour_frag_image (include/nerficg_hip.h group 30): the builder that nrc_ngp_render_frame runs for the colour net's fragment image, on its own.
The 14 336 bytes it writes are BYTE-equal to the numpy restatement (tests/colour_frag_image_ref.py) on 7 168 distinct halves, so every byte says which
weight it came from; the 256 guard bytes behind the image stay untouched."""
import numpy as np
import pytest
import torch

from tests import colour_frag_image_ref as ref

DEV = 'cuda'
pytestmark = pytest.mark.gpu


def test_image_content():
    from nerficg_amd import _lib
    lib = _lib.load()
    w = ref.distinct_weights()
    wc = torch.from_numpy(w).to(DEV)
    out = torch.full((14336 + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    _lib.check(lib.nrc_ngp_colour_frag_image(_lib.ptr(wc), _lib.ptr(out), _lib.stream_of(wc)), 'ngp_colour_frag_image')
    got = out.cpu().numpy()
    want = ref.image_of(w)
    assert want.nbytes == 14336
    assert np.array_equal(got[:14336], np.frombuffer(want.tobytes(), np.uint8))
    assert (got[14336:] == 0xA5).all()   # nothing behind the image
    assert lib.nrc_ngp_colour_frag_image(None, _lib.ptr(out), _lib.stream_of(wc)) == -1
    assert lib.nrc_ngp_colour_frag_image(_lib.ptr(wc), None, _lib.stream_of(wc)) == -1
