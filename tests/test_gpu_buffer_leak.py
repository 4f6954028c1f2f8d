"""ldpc_hip_bp_destroy frees every device buffer a handle grew: the library's own count of the bytes its DeviceBufs hold
(ldpc_hip_debug_device_buf_bytes -- free memory as the runtime reports it is no witness on a GPU other work shares) is the same after
create / decode / close as before.  One case per family of buffers that are built on first use: the item form of the serial schedule
with its tile kernel (ser_var_*), serial_relative with its state beyond LDS (rl_first, rl_rec, rl_ext_A), and BP + OSD on the default
parallel schedule.  With the hand-kept release lists this replaces, the first two cases fail: 5 625 224 and 5 415 168 bytes
outlive the handle at these sizes; the third passes there too."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _syndromes(h, batch, p, seed):
    rng = np.random.default_rng(seed)
    errors = (rng.random((batch, h.shape[1])) < p).astype(np.uint8)
    return np.ascontiguousarray((errors @ h.T.toarray().astype(np.uint8)) & 1, np.uint8)


def _serial_item_form():
    from ldpc_amd import codes
    h = codes.irregular_ldpc_code(2400, 1200, seed=1)

    def setup(eng):
        eng.set_schedule("serial")
        eng.set_serial_kernel(2)  # the streamed kernels whatever the width of the levels: this matrix takes the item form
    return h, dict(p=0.03, max_iter=20, method=0, alpha=1.0, batch=320), setup, {}  # > 256 rows: the tile kernel and its tables


def _serial_relative_ext():
    from ldpc_amd import codes
    h = codes.hypergraph_product_hx(codes.regular_ldpc_code(n=32, dv=3, dc=4, seed=5))
    return h, dict(p=0.02, max_iter=30, method=1, alpha=0.625, batch=96), lambda eng: eng.set_schedule("serial_relative"), {}


def _parallel_bposd():
    from ldpc_amd import codes
    h = codes.regular_ldpc_code(n=96, dv=3, dc=6, seed=3)
    return h, dict(p=0.08, max_iter=8, method=1, alpha=0.625, batch=200), lambda eng: eng.set_osd(1, 0), dict(osd=True)


@pytest.mark.parametrize("case", [_serial_item_form, _serial_relative_ext, _parallel_bposd], ids=lambda f: f.__name__.strip("_"))
def test_close_frees_every_device_buffer(case):
    from ldpc_amd import _lib
    from ldpc_amd.engine import HipBpEngine
    h, c, setup, decode_args = case()
    h = h.tocsr()
    h.sort_indices()
    held = _lib.load().ldpc_hip_debug_device_buf_bytes
    before = held()
    eng = HipBpEngine(h.indptr, h.indices, h.shape[1], np.full(h.shape[1], c["p"]), c["max_iter"], c["method"], c["alpha"])
    setup(eng)
    eng.decode_batch(_syndromes(h, c["batch"], c["p"], seed=11), **decode_args)
    during = held()
    eng.close()
    after = held()
    print(f"{case.__name__}: device buffer bytes before {before}, with the engine {during}, after close {after}")
    assert during > before, "the decode went through no counted buffer: the test would see no leak"
    assert after == before, f"{after - before} bytes of device buffers outlive the handle"
