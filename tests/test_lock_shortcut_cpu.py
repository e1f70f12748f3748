"""sidecar_amd.dist.lock_shortcut: when a sharded push-pull round with every host locked may be replaced
by its counts (gx_ae_skip_locked). With lock_readers an exchange between read-locked hosts runs, so an
all-locked round is not a round of failures and the shortcut is off."""
import pytest

from sidecar_amd.abi import default_params
from sidecar_amd.dist import lock_shortcut

_KW = dict(n_hosts=32, n_services=4, ae_period_rounds=1)


@pytest.mark.parametrize("change,want", [
    (dict(), True),
    (dict(push_pull_mode=1, push_pull_stagger=1), True),
    (dict(depart_round=4), True),  # no host departs at 0 ppm
    (dict(depart_round=-1, depart_ppm=1000), True),
    (dict(lock_model=0), False),
    (dict(fd_enable=1), False),
    (dict(depart_round=4, depart_ppm=1000), False),
    (dict(depart_round=0, depart_ppm=1), False),
])
def test_lock_shortcut_without_lock_readers(oracle_lib, change, want):
    assert lock_shortcut(default_params(oracle_lib, **_KW, **change)) is want
    assert lock_shortcut(default_params(oracle_lib, lock_readers=0, **_KW, **change)) is want


@pytest.mark.parametrize("change", [dict(), dict(lock_readers=2), dict(push_pull_mode=1), dict(lock_defer_slots=8),
                                    dict(depart_round=4, depart_ppm=1000)])
def test_lock_shortcut_is_off_with_lock_readers(oracle_lib, change):
    assert lock_shortcut(default_params(oracle_lib, **{**_KW, "lock_readers": 1, **change})) is False
