"""The trainer's log lines against its own loss calls on HipOps (tests/metric_record_cases.py, the tiny golden model)."""
import pytest

import metric_record_cases as mrc

pytestmark = pytest.mark.gpu


def test_logged_values_are_the_loss_calls_on_hip(hip_ops, tmp_path):
    mrc.check_logged_values_are_the_loss_calls(hip_ops, tmp_path)
