"""ellp_engine_dual_rephase on a tall, narrow LP: A_B is too large for the engine's slab of small allocations and A_N is the
slab's first tenant, so A_N has the slab's own address.  Re-ordering N into variable order replaces A_N (replace_alloc);
that must not release the slab, which holds b, the bounds and every other small array of the engine (it did: the copy of the
new right-hand side then failed with "invalid argument")."""
import pytest

from oracle import ellp_oracle as eo
from test_gpu_dual_rephase import _case

pytestmark = pytest.mark.gpu


def test_dual_rephase_when_the_nonbasic_columns_open_the_slab():
    # 300 x 20: A_B is 304^2 doubles (0.7 MB, outside the slab), A_N 20 columns (48 KB, the slab's first allocation)
    st, it_g, it_o = _case(eo.synth_problem(9, 300, 20))
    assert st == eo.OPTIMAL
