#!/usr/bin/env python3
"""Which of the library's kernel instantiations a run launched: the compiled names from the resource-usage listing against a launch log.
    make -C ldpc_amd/csrc resource-usage > /tmp/ru.txt 2>&1
    LDPC_HIP_LAUNCH_LOG=/tmp/launches.txt python -m pytest tests -m gpu          (the log: profiles/README.md)
    python tools/instantiation_coverage.py /tmp/ru.txt /tmp/launches.txt [more logs ...] > profiles/instantiation_coverage.txt
Prints reached / total per template and every unreached name.  In the families the instantiation tests walk -- tests/test_gpu_instantiations.py
(bp_edge_kernel, bp_edge8_kernel, bp_wave_kernel, bp_wave_ps_kernel), tests/test_gpu_row_priors_edge.py (bp_edge_rp_kernel, bp_edge8_rp_kernel) and
tests/test_gpu_stream_instantiations.py (the streamed, per-pass, serial and slot kernels: WALKED below) -- an unreached name is marked: "not selectable"
where no host rule can pick it (NOT_SELECTABLE below, with the reason), else "gap"; the other families are listed only."""
import re
import subprocess
import sys

WALKED = ("bp_edge_kernel", "bp_edge8_kernel", "bp_wave_kernel", "bp_wave_ps_kernel", "bp_edge_rp_kernel", "bp_edge8_rp_kernel",
          "bp_decode_kernel", "bp_spread_check_kernel", "bp_spread_bit_kernel", "bp_spread_init_kernel", "bp_spread_finish_kernel", "bp_spread_synd_kernel",
          "bp_edge0_kernel", "bp_relative_lds_kernel", "bp_serial_relative_kernel", "bp_serial_kernel", "bp_serial_level_kernel", "bp_serial_stream_kernel",
          "bp_serial_stream_var_kernel", "bp_serial_lane_kernel", "bp_serial_lane_var_kernel", "serial_edge0_kernel", "serial_var_init_kernel", "bp_small_kernel")
# instantiation -> why no rule selects it (tests/stream_ladder_util.py NOT_SELECTABLE names the case that keeps each claim true; tests/ladder_util.py
# UNREACHABLE would hold those of the wavefront ladders)
NOT_SELECTABLE = {
    "bp_decode_kernel<1, 0, 4, 3, 2>": "tu_stream.hip pick_kernel: the (3,4)-regular ring is product-sum only; min-sum at ring 2 runs <1, 0, 4, 3, 0> "
                                       "(test_streamed_kernel_instantiation[decode-ms-ring2-4x3])",
    "bp_decode_kernel<1, 0, 5, 3, 2>": "tu_stream.hip pick_kernel: the (3,5)-regular ring is product-sum only; min-sum at ring 2 runs <1, 0, 6, 3, 0> "
                                       "(test_streamed_kernel_instantiation[decode-ms-ring2-5x3])",
}
# templates whose second argument is MATH (<METHOD, MATH, ...>); bp_wave_ps_kernel<MATH, ...> is product-sum only
METHOD_MATH = ("bp_wave_kernel", "bp_decode_kernel", "bp_spread_check_kernel", "bp_spread_bit_kernel", "bp_spread_init_kernel", "bp_edge0_kernel",
               "bp_relative_lds_kernel", "bp_serial_relative_kernel", "bp_serial_kernel", "bp_serial_level_kernel", "bp_serial_stream_kernel",
               "bp_serial_stream_var_kernel", "bp_serial_lane_kernel", "bp_serial_lane_var_kernel", "serial_edge0_kernel", "serial_var_init_kernel", "bp_small_kernel")


def fast_math(name):
    """A <METHOD, MATH, ...> instantiation (or bp_wave_ps_kernel<MATH, ...>) with MATH = 1: selectable through ldpc_hip_bp_set_math."""
    base = name.split("<")[0]
    args = [a.strip() for a in name[name.index("<") + 1:-1].split(",")]
    return (base in METHOD_MATH and args[1] == "1") or (base == "bp_wave_ps_kernel" and args[0] == "1")


def compiled_names(listing):
    mangled = re.findall(r"remark: Function Name: (\S+)", open(listing).read())
    dem = subprocess.run(["c++filt"] + mangled, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    return sorted({d.replace("void ", "").split("(")[0] for d in dem})


def launched_names(logs):
    counts = {}
    for path in logs:
        for line in open(path):
            if line.startswith("#") or "\t" not in line:
                continue
            count, name = line.rstrip("\n").split("\t", 1)
            counts[name] = counts.get(name, 0) + int(count)
    return counts


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    compiled, launched = compiled_names(argv[1]), launched_names(argv[2:])
    groups = {}
    for name in compiled:
        groups.setdefault(name.split("<")[0], []).append(name)
    reached = [n for n in compiled if n in launched]
    print(f"# {len(reached)} of {len(compiled)} kernel instantiations of libldpc_hip.so launched ({sum(launched.values())} launches in the log)")
    unknown = sorted(set(launched) - set(compiled))
    if unknown:
        print(f"# launched but not in the listing ({len(unknown)}): " + "; ".join(unknown))
    print("\n# reached / compiled per template")
    for base in sorted(groups, key=lambda k: (-len(groups[k]), k)):
        hit = sum(n in launched for n in groups[base])
        print(f"{hit:4d} / {len(groups[base]):3d}  {base}")
    print("\n# unreached instantiations")
    for base in sorted(groups, key=lambda k: (-len(groups[k]), k)):
        missing = [n for n in groups[base] if n not in launched]
        if not missing:
            continue
        print(f"\n## {base}  ({len(missing)} of {len(groups[base])} unreached)")
        for n in missing:
            mark = ""
            if base in WALKED:
                mark = (f"   <-- not selectable by any rule: {NOT_SELECTABLE[n]}" if n in NOT_SELECTABLE
                        else "   <-- gap: fast math" if fast_math(n) else "   <-- gap")
            print(f"   {n}{mark}")


if __name__ == "__main__":
    main(sys.argv)
