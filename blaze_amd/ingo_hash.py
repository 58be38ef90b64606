"""Host-side mirror of src/ingo_hash (poseidon_api.rs, utils.rs): same names and call sequence over the C ABI.
include/blaze_hip.h "Poseidon" states the hash, the tree, the record and what the instruction CSV means here."""
from __future__ import annotations

import ctypes as C
import enum
import logging
from dataclasses import dataclass
from typing import Optional

from ._lib import DeviceBuffer, buf_ptr, check, lib
from .driver_client import DriverClient, DriverPrimitive

log = logging.getLogger(__name__)


class Hash(enum.Enum):  # poseidon_api.rs:11-13
    Poseidon = 0


class TreeMode(enum.IntEnum):  # utils.rs:16-30
    TreeC = 0
    TreeD = 1

    @staticmethod
    def value_of(tree_mode: "TreeMode") -> int:  # TreeMode::value
        return int(tree_mode)


def num_of_elements_oct_tree(tree_height: int) -> int:  # utils.rs:2-10
    return sum(8 ** (tree_height - i - 1) for i in range(tree_height))


def num_of_elements_in_base_layer(tree_height: int) -> int:  # utils.rs:12-14
    return 8 ** (tree_height - 1)


@dataclass
class PoseidonInitializeParameters:  # poseidon_api.rs:19-24
    tree_height: int
    tree_mode: TreeMode
    instruction_path: str


@dataclass
class PoseidonResult:  # poseidon_api.rs:26-30
    hash_byte: bytes
    hash_id: int
    layer_id: int

    @staticmethod
    def parse_poseidon_hash_results(data) -> list["PoseidonResult"]:  # poseidon_api.rs:42-71
        data = bytes(data)
        if len(data) % 64:
            raise ValueError("records are 64 bytes each")
        out = []
        for k in range(0, len(data), 64):
            hash_data = data[k + 32:k + 64]
            hash_id = int.from_bytes(hash_data[:4], "little") & 0x3FFFFFFF
            layer_id = int.from_bytes(hash_data[3:5], "little") >> 6
            out.append(PoseidonResult(data[k:k + 32], hash_id, layer_id))
        return out


@dataclass
class PoseidonImageParametrs:  # poseidon_api.rs:256-278
    hif2_cpu_c_is_stub: int
    hif2_cpu_c_number_of_cores: int
    hif2_cpu_c_place_holder: int

    @staticmethod
    def parse_image_params(params: int) -> "PoseidonImageParametrs":
        # params.to_be_bytes(), packed_struct msb0: bit k of the buffer is bit 31 - k of the word
        return PoseidonImageParametrs(params & 0xF, (params >> 4) & 0xFF, (params >> 12) & 0xFFFFF)


class PoseidonClient(DriverPrimitive[Hash, PoseidonInitializeParameters, bytes, list]):
    """poseidon_api.rs:15-17, 74-254.  `field` names the curve whose scalar field the hash is over ("BLS381", the field of the
    reference's TEST_SCALAR, by default)."""

    _FIELDS = {"BLS377": 0, "BLS381": 1, "BN254": 2}  # enum blz_curve

    def __init__(self, _ptype: Hash, dclient: DriverClient, field: str = "BLS381"):
        self.driver_client = dclient
        self.field = field
        h = C.c_void_p()
        check(lib().blz_poseidon_new(dclient.id, self._FIELDS[field], C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().blz_poseidon_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def loaded_binary_parameters(self) -> list[int]:  # poseidon_api.rs:81-94
        v = (C.c_uint32 * 2)()
        check(lib().blz_poseidon_loaded_binary_parameters(self._h, v))
        return [int(v[0]), int(v[1])]

    def initialize(self, param: PoseidonInitializeParameters) -> None:  # poseidon_api.rs:96-111
        check(lib().blz_poseidon_initialize(self._h, param.tree_height, int(param.tree_mode), param.instruction_path.encode()))

    def initialize_words(self, tree_height: int, tree_mode: TreeMode, words) -> None:
        """initialize with the instruction word stream from memory (32-byte little-endian words)"""
        p, n, _k = buf_ptr(words)
        check(lib().blz_poseidon_initialize_words(self._h, tree_height, int(tree_mode), p, n))

    def start_process(self, _param: Optional[int] = None) -> None:
        raise NotImplementedError("todo!() in the reference too (poseidon_api.rs:113-115)")

    def set_data(self, input) -> None:  # poseidon_api.rs:117-122
        if isinstance(input, DeviceBuffer):
            check(lib().blz_poseidon_set_data_device(self._h, input.ptr, input.nbytes))
            return
        p, n, _k = buf_ptr(input)
        check(lib().blz_poseidon_set_data(self._h, p, n))

    def wait_result(self) -> None:
        """todo!() in the reference (poseidon_api.rs:124-126); here: every node whose inputs have arrived is hashed when it returns"""
        check(lib().blz_poseidon_wait_result(self._h))

    def result(self, expected_result: Optional[int] = None) -> Optional[list]:  # poseidon_api.rs:128-145
        if expected_result is None:
            raise TypeError("expected_result is required (the reference unwraps it: poseidon_api.rs:134)")
        out = bytearray(64 * expected_result)
        p, _, _k = buf_ptr(out)
        n = C.c_uint32()
        check(lib().blz_poseidon_result(self._h, expected_result, p, len(out), C.byref(n)))
        return PoseidonResult.parse_poseidon_hash_results(out[: 64 * n.value])

    def get_num_of_pending_results(self) -> int:  # poseidon_api.rs:156-161
        v = C.c_uint32()
        check(lib().blz_poseidon_num_pending_results(self._h, C.byref(v)))
        return int(v.value)

    def get_raw_results(self, num_of_results: int) -> bytearray:  # poseidon_api.rs:191-196
        out = bytearray(64 * num_of_results)
        p, _, _k = buf_ptr(out)
        check(lib().blz_poseidon_raw_results(self._h, num_of_results, p, len(out)))
        return out

    def _counters(self) -> list[int]:
        v = (C.c_uint32 * 4)()
        check(lib().blz_poseidon_counters(self._h, v))
        return [int(x) for x in v]

    def get_last_element_sent_to_ring(self) -> int:  # poseidon_api.rs:149-154
        return self._counters()[0]

    def get_last_hash_sent_to_host(self) -> int:  # poseidon_api.rs:198-203
        return self._counters()[1]

    def log_api_values(self) -> None:  # poseidon_api.rs:245-253
        c = self._counters()
        log.debug("=== api values === elements %d, last hash id %d, last layer %d, elements waiting %d, pending results %d", *c,
                  self.get_num_of_pending_results())

    def tree_device(self, dst: DeviceBuffer) -> None:
        """every record of the finished tree, (layer, id) order, into a device buffer (blz_poseidon_tree_device)"""
        check(lib().blz_poseidon_tree_device(self._h, dst.ptr, dst.nbytes))

    def info(self) -> dict:
        v = (C.c_uint64 * 4)()
        check(lib().blz_poseidon_info(self._h, v))
        return {"device_bytes": int(v[0]), "optimised_partial_rounds": bool(v[1]), "round_plan_check": int(v[2]), "width_mask": int(v[3])}

    def set_round_plan(self, enable: bool) -> None:
        check(lib().blz_poseidon_set_round_plan(self._h, 1 if enable else 0))

    def prepare_round_plan(self) -> dict:
        """derive and self-check the optimised partial rounds now, not under the first tree (blz_poseidon_prepare_round_plan);
        the two words info() reports: in force, and the self-check's state (0 not run, 1 equal, 2 refused: dense rounds)"""
        v = (C.c_uint32 * 2)()
        check(lib().blz_poseidon_prepare_round_plan(self._h, v))
        return {"optimised_partial_rounds": bool(v[0]), "round_plan_check": int(v[1])}

    def last_kernel_ms(self) -> float:
        v = C.c_float()
        check(lib().blz_poseidon_last_kernel_ms(self._h, C.byref(v)))
        return float(v.value)

    def reset(self) -> None:
        check(lib().blz_poseidon_reset(self._h))


def check_words(field: str, tree_mode: TreeMode, words) -> dict:
    """The load-time checks of the instruction word stream, host side only (blz_poseidon_check_words)."""
    p, n, _k = buf_ptr(words)
    v = (C.c_uint32 * 4)()
    check(lib().blz_poseidon_check_words(PoseidonClient._FIELDS[field], int(tree_mode), p, n, v))
    # (word 2 is always 0: whether the widths admit the optimised rounds is PoseidonClient.prepare_round_plan's answer)
    return {"blocks": int(v[0]), "width_mask": int(v[1]), "optimised_partial_rounds": bool(v[2]), "words": int(v[3])}
