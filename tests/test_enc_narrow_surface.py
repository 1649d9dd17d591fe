"""encode_tensors(wire_dtype=...): the argument checks, which precede every use of the device."""
import pytest

torch = pytest.importorskip("torch")
from psyne_amd.tdt import TdtCodec  # noqa: E402


@pytest.mark.parametrize("others", [{"packed": True}, {"word_sizes": "dtype"}, {"mapbits": torch.zeros(1, dtype=torch.int64)},
                                    {"exact": True}, {"return_mappings": True}])
def test_wire_dtype_combines_with_nothing(others):
    codec = TdtCodec.__new__(TdtCodec)  # (no context: the checks come first)
    with pytest.raises(ValueError, match="wire_dtype does not combine with " + next(iter(others))):
        codec.encode_tensors([torch.zeros(8)], wire_dtype=torch.bfloat16, **others)


def test_wire_dtype_takes_float32_tensors_and_two_types():
    codec = TdtCodec.__new__(TdtCodec)
    with pytest.raises(ValueError, match="narrows float32 tensors"):
        codec.encode_tensors([torch.zeros(8, dtype=torch.float16)], wire_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="wire_dtype is torch.bfloat16"):
        codec.encode_tensors([torch.zeros(8)], wire_dtype=torch.float64)
