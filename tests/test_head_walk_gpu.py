"""GPU (-m gpu): test_head_walk's accumulator cases on the device, for both flag values of losses._HeadGrads -- the bf16 GEMMs of
the cross-entropy and per-sequence nodes and the fp32-output GEMMs of the Cosy node, which torch implements on the GPU alone.
torch.equal against the nodes' former loops restated in test_head_walk: the same library calls on the same shapes and strides."""
import pytest

from test_head_walk import NEEDS, accumulator_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("need", NEEDS)
def test_accumulator_equals_the_nodes_own_loops(need, with_bias, fp32):
    accumulator_case(DEV, fp32, need, with_bias)


@pytest.mark.parametrize("fp32", [False, True])
def test_accumulator_on_a_zero_padded_weight(fp32):
    accumulator_case(DEV, fp32, (True, True, True), False, padded=True)


def test_accumulator_takes_db_from_the_fp32_rows_of_a_torch_route():
    accumulator_case(DEV, False, (True, True, True), True, from_fp32=True)
