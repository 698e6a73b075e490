"""The trainer's log lines against its own loss calls on the CPU op backend (tests/metric_record_cases.py)."""
import metric_record_cases as mrc
from oracle.ref_ops import RefOps


def test_logged_values_are_the_loss_calls(tmp_path):
    mrc.check_logged_values_are_the_loss_calls(RefOps(), tmp_path)
