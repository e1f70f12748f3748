"""The sharded push-pull chain refuses calls that arrive out of order or with the wrong size
(GX_EINVAL, before anything is launched or read), answers empty in a round or past a batch with
nothing to run, and a refused call leaves nothing behind: the round finishes with the right calls
and the shards stay bit-identical to the unsharded engine. The table is tests/ae_chain_order_cases.py."""
import pytest

from tests.ae_chain_order_cases import CASES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__)
def test_gpu_ae_chain_order(gx_lib, case):
    case(gx_lib)
