"""tests/test_mexcache_keys.py on real hardware: the shims built against libsedumi_hip.so (the fixtures of tests/test_mexshims_gpu.py)."""
import pytest

from test_mexcache_keys import test_each_key_component_rebuilds_exactly_the_slots_keyed_on_it  # noqa: F401
from test_mexshims_gpu import _hip, shimlib, shimmex  # noqa: F401

pytestmark = pytest.mark.gpu
