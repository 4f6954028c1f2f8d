"""What a decode launched, from the library's launch log (ldpc_amd.engine.launch_log, ldpc_hip_debug_launch_log): helpers for the tests
that name a kernel and want to SEE that it ran.  Names are spelt as tools/list_instantiations.py spells them: "bp_edge8_kernel<12, 3, true>"."""
from ldpc_amd.engine import launch_log  # noqa: F401  (with launch_log() as log: ...; log is filled when the block is left)


def base(name):
    """Template name of an instantiation: "bp_edge8_kernel<12, 3, true>" -> "bp_edge8_kernel"."""
    return name.split("<")[0]


def of(log, *bases):
    """The logged instantiations of the given templates, sorted."""
    return sorted(k for k in log if base(k) in bases)


def assert_resolved(log):
    assert log, "the launch log is empty: nothing was launched inside the block"
    unnamed = [k for k in log if k.startswith("?")]
    assert not unnamed, f"launched kernels without a name: {unnamed}"


def assert_ran(log, *names):
    """Every name -- an instantiation, or a template's base name -- was launched."""
    assert_resolved(log)
    for name in names:
        hit = name in log if "<" in name else bool(of(log, name))
        assert hit, f"{name} was not launched; the log has {sorted(log)}"


def assert_not_ran(log, *names):
    assert_resolved(log)
    for name in names:
        hit = [name] if name in log else [] if "<" in name else of(log, name)
        assert not hit, f"{hit} launched, against expectation; the log has {sorted(log)}"
