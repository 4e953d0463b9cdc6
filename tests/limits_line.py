"""The two lines tests/host_c/limits_sweep --print writes, parsed in one place (tests/test_limits_host.py, tests/test_gpu_value_range.py)."""
import re

LIMITS_LINE = re.compile(r"limits: sys_ok (\d+) pk_kmax (\d+) pk16_kmax (\d+) \(f16 up to (\d+)\) chunk cap (\d+)")
SHAPES_LINE = re.compile(r"shapes: pk_kmax (\d+) pk16_kmin (\d+) pk16_kmax (\d+) pk16_f16_kmax (\d+) pk_wpb (\d+) sys_chunk (\d+) long_w (\d+)")


def parse_limits(out: str) -> dict:
    """the `limits:` line of limits_sweep --print"""
    m = LIMITS_LINE.search(out)
    assert m, out
    return dict(zip(("sys_ok", "pk", "pk16", "f16", "chunk_cap"), map(int, m.groups())))


def parse_shapes(out: str) -> dict:
    m = SHAPES_LINE.search(out)
    assert m, out
    return dict(zip(("pk_kmax", "pk16_kmin", "pk16_kmax", "pk16_f16_kmax", "pk_wpb", "sys_chunk", "long_w"), map(int, m.groups())))
