#!/usr/bin/env python3
"""Generate tests/golden/reference_abi.json: the binary interface of the reference's generated solver headers
(plan_manage/solver/{normal,final}/FORCESNLPsolver_*/include/FORCESNLPsolver_*.h:110-323), as numbers and canonical type
spellings only -- struct sizes, field offsets and sizes, the exit codes the caller distinguishes, the callback type and the
solve prototype.  Run where the reference tree is, with its root as the argument; nothing from the headers is copied, a
program compiled against them prints what the compiler sees.  tests/test_capi_cpu.py checks include/frp_nmpc.h against it.

  python tests/tools/gen_reference_abi.py REFERENCE_ROOT
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "reference_abi.json")
FIELDS = {"params": ["xinit", "x0", "all_parameters", "num_of_threads"],
          "output": ["x01", "x02", "x20"],
          "info": ["it", "it2opt", "res_eq", "res_ineq", "rsnorm", "rcompnorm", "pobj", "dobj", "dgap", "rdgap", "mu", "mu_aff", "sigma",
                   "lsit_aff", "lsit_cc", "step_aff", "step_cc", "solvetime", "fevalstime"]}
EXIT_CODES = ["OPTIMAL", "MAXITREACHED", "FACTORIZATION_ERROR", "BADFUNCEVAL", "NOPROGRESS", "PARAM_VALUE_ERROR", "LICENSE_ERROR"]


def probe(ref, m):
    R = f"FORCESNLPsolver_{m}"
    inc = os.path.join(ref, "src", "resilient_planner", "plan_manage", "solver", m, R, "include")
    lines = [f'#include "{R}.h"', "#include <cstddef>", "#include <cstdio>",
             "template <class T> const char *tn() { return __PRETTY_FUNCTION__; }  // '... [with T = <canonical type>]'",
             "int main() {", '    printf("{");']
    for s, names in FIELDS.items():
        lines.append(f'    printf("\\"{s}\\": {{\\"size\\": %zu, \\"fields\\": {{", sizeof({R}_{s}));')
        for i, f in enumerate(names):
            sep = ", " if i else ""
            lines.append(f'    printf("{sep}\\"{f}\\": [%zu, %zu]", offsetof({R}_{s}, {f}), sizeof((({R}_{s} *)0)->{f}));')
        lines.append('    printf("}}, ");')
    lines.append('    printf("\\"exit_codes\\": {");')
    for i, c in enumerate(EXIT_CODES):
        sep = ", " if i else ""
        lines.append(f'    printf("{sep}\\"{c}\\": %d", (int){c}_{R});')
    lines.append('    printf("}, ");')
    lines.append(f'    printf("\\"extfunc\\": \\"%s\\", ", tn<{R}_extfunc>());')
    lines.append(f'    printf("\\"solve\\": \\"%s\\"}}\\n", tn<decltype(&{R}_solve)>());')
    lines.append("    return 0;\n}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.cpp"), os.path.join(d, "probe")
        open(src, "w").write("\n".join(lines) + "\n")
        subprocess.check_call(["g++", "-std=c++17", "-I" + inc, src, "-o", exe, "-Wl,--unresolved-symbols=ignore-all"])
        rec = json.loads(subprocess.check_output([exe], text=True))
    for k in ("extfunc", "solve"):
        rec[k] = rec[k][rec[k].index("T = ") + 4:rec[k].rindex("]")]
    # the struct names of the prototype are the header's own: stored as {solver}_params etc.
    rec["solve"] = rec["solve"].replace(R + "_", "{solver}_")
    return rec


def main():
    ref = sys.argv[1]
    out = {"what": "binary interface of the reference's FORCESNLPsolver_{normal,final}.h as a compiler sees it (tests/tools/gen_reference_abi.py): "
                   "sizes and [offset, size] of the fields in bytes, exit-code values, canonical callback / solve types",
           "models": {m: probe(ref, m) for m in ("normal", "final")}}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
