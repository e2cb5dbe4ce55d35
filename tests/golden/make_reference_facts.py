"""Records the facts about the reference's Lua scripts that the CPU tests check, into reference_facts.json.

The tests must run from a checkout of this project alone, so they read these recorded facts instead of the reference
tree.  Nothing of the reference's program text is stored: only option names with their defaults, the defaults of the
two setTestArgs methods, and -- for the statements lua/run_model_hip.lua substitutes -- a SHA-256 of each statement
with the number of times it occurs in run_model.lua.
Run:  python tests/golden/make_reference_facts.py <path of a jcjohnson/densecap checkout>
"""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CLI_SCRIPTS = ("run_model.lua", "extract_features.lua", "webcam/daemon.lua")
OPTION = r"cmd:option\('(-\w+)',\s*\n?\s*('[^']*'|[\d.]+)"
GETOPT = r"getopt\((?:kwargs|args),\s*'(\w+)',\s*([\w.]+)\)"


def substitution_patterns():
    """The (Lua pattern, replacement) pairs of lua/run_model_hip.lua."""
    lua = open(os.path.join(ROOT, "lua", "run_model_hip.lua")).read()
    return re.findall(r'\{"((?:[^"\\]|\\.)*)",\s*\n\s*"((?:[^"\\]|\\.)*)"\}', lua)


def pattern_literal(pat):
    return re.sub(r"%(.)", r"\1", pat)          # Lua escapes a magic character with %


def sha256(text):
    return hashlib.sha256(text.encode()).hexdigest()


def _function_body(src, header):
    i = src.index(header)
    return src[i:i + re.search(r"\nend\b", src[i:]).start()]


def main(ref):
    facts = {"_source": "jcjohnson/densecap: %s, densecap/DenseCapModel.lua, densecap/LocalizationLayer.lua "
                        "(made by make_reference_facts.py)" % ", ".join(CLI_SCRIPTS)}
    facts["cli_options"] = {}
    for name in CLI_SCRIPTS:
        found = re.findall(OPTION, open(os.path.join(ref, name)).read())
        facts["cli_options"][name] = {k: v.strip("'") for k, v in found}
    model = _function_body(open(os.path.join(ref, "densecap", "DenseCapModel.lua")).read(),
                           "function DenseCapModel:setTestArgs(kwargs)")
    layer = _function_body(open(os.path.join(ref, "densecap", "LocalizationLayer.lua")).read(),
                           "function layer:setTestArgs(args)")
    facts["set_test_args_defaults"] = {"DenseCapModel": dict(re.findall(GETOPT, model)),
                                       "LocalizationLayer": dict(re.findall(GETOPT, layer))}
    text = open(os.path.join(ref, "run_model.lua")).read()
    facts["run_model_statement_counts"] = {sha256(pattern_literal(p)): text.count(pattern_literal(p))
                                           for p, _ in substitution_patterns()}
    with open(os.path.join(HERE, "reference_facts.json"), "w") as f:
        json.dump(facts, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
