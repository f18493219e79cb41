"""GPU: mumpy_dwconv5_window_bwd stays inside its buffers when C is not a multiple of 64 (Cg = 32 at C = 96, every cross-view block of
stage 1).  Its db reduce used to bound the column index by the row stride of the partials (26 C) instead of its own C columns: the
launch's one block wrote 32 floats past db and read 32 floats past the end of the workspace.  Here db, dw and the workspace are
slices in the middle of one large buffer, so a stray access would stay inside memory the test owns; the test asserts there is none."""
import pytest
import torch

from weight_fill import seeded_randn

pytestmark = pytest.mark.gpu
FILL = 12345.0


@pytest.mark.parametrize("n,c", [(6, 32), (2, 32), (3, 96), (5, 128)])
def test_dwconv5_bwd_reduce_stays_inside_db_and_the_workspace(n, c):
    from mumpy_hip.lib import load_library
    lib = load_library()
    dev = "cuda"
    x, du, w = seeded_randn(100, n, 49, c).to(dev), seeded_randn(103, n, 49, c).to(dev), (seeded_randn(101, c, 25) / 5).to(dev)
    wsb = int(lib.mumpy_dwconv5_window_bwd_workspace_bytes(n, c))
    assert wsb == n * 26 * c * 4

    def run(tail_value):
        big = torch.full((1 << 18,), FILL, device=dev)
        dx = torch.empty_like(x)
        o_dw, o_db, o_ws = 4096, 65536, 131072
        dw, db, ws = big[o_dw:o_dw + 26 * c], big[o_db:o_db + c], big[o_ws:o_ws + wsb // 4]
        big[o_ws + wsb // 4:o_ws + wsb // 4 + 256] = tail_value                 # what a read past the workspace would pick up
        rc = lib.mumpy_dwconv5_window_bwd(x.data_ptr(), w.data_ptr(), du.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                          ws.data_ptr(), wsb, n, c, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0
        before_db, after_db = big[o_db - 256:o_db], big[o_db + c:o_db + c + 256]
        assert bool((before_db == FILL).all()) and bool((after_db == FILL).all()), "the db reduce wrote outside db"
        assert bool((big[o_dw - 256:o_dw] == FILL).all()) and bool((big[o_dw + 26 * c:o_dw + 26 * c + 256] == FILL).all())
        assert bool((big[o_ws - 256:o_ws] == FILL).all())
        return db.clone(), dw[:25 * c].clone()
    db_a, dw_a = run(1000.0)
    db_b, dw_b = run(-7.0)
    assert torch.equal(db_a, db_b) and torch.equal(dw_a, dw_b)                  # nothing past the workspace reaches a result
    ref_db = du.double().sum((0, 1))
    assert float((db_a.double() - ref_db).abs().max() / ref_db.abs().max()) < 5e-5
