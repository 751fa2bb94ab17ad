"""CPU-only check of csrc/derived_state.h, the table of what a solver handle derives from its inputs: the stand-alone
program tests/derived_state_main.cpp sets every flag, calls each cause and prints which flags fell; this module states,
in its own words, which inputs each item was computed from and which inputs each cause changes, and expects a flag to
fall exactly where the two sets meet."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

# what each item was computed from.  sweep: the handle runs the single-sweep erm iteration on an unbroken chain of rho
# predictions (the look-ahead exists only there)
ITEM_INPUTS = {
    "v_valid": {"D", "w"},                                                   # v = D w
    "z_ready": {"D", "y", "w", "z", "lam", "rho", "rw", "sweep"},            # z_next, q, ||z_next||^2 of the next iteration
    "p_valid": {"D", "y", "lam", "sweep"},                                   # p = D^T lambda (own labels change the stored lambda)
    "p_pending": {"D", "y", "lam", "sweep"},                                 # a fresh D^T lambda waiting to become p
    "pred_valid": {"D", "y", "w", "z", "lam", "rho", "rw", "G", "sweep"},    # rho predicted from q, p, G w and the norms
    "keys_ready": {"D", "y", "w", "lam", "rho"},                             # sort keys of m = D w - lambda / rho
    "s32_m_ready": {"D", "y", "w", "lam", "rho"},                            # m and its range
    "s32_used": {"D", "y", "w", "z", "lam", "rho"},                          # an unread verdict on z, redone from m
    "s32_q_done": {"D", "y", "w", "z", "lam", "rho"},
    "zb_used": {"D", "y", "w", "z", "lam", "rho"},
    "zb_q_done": {"D", "y", "w", "z", "lam", "rho"},
    "zb_c_ready": {"z", "lam", "rho"},                                       # c = z + lambda / rho
    "gram_local_done": {"D"},                                                # G = D^T D of the handle's rows
    "gram_ready": {"D", "G"},                                                # G whole, L taken from it
    "eig_ok": {"G"},                                                         # the eigenbasis of G
}
# what each cause changes
CAUSE_INPUTS = {
    "data_changed": {"D", "y", "G"},      # an upload: D = -y X, and the G that stands belongs to the old D
    "w_changed": {"w"},
    "z_replaced": {"z"},
    "lambda_changed": {"lam"},
    "rho_changed": {"rho"},
    "labels_changed": {"y"},
    "row_weights_changed": {"rw"},
    "gram_changed": {"G"},
    "drop_look_ahead": {"sweep"},
}


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("derived_state") / "derived_state_main")
    src = os.path.join(ROOT, "tests", "derived_state_main.cpp")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    cc = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and ("cannot find" in cc.stderr or "unsupported" in cc.stderr):
        cc = subprocess.run(base + [src, "-o", exe], capture_output=True, text=True)   # no sanitizer runtimes: the table is still checked
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "derived_state: done" in run.stdout and "FAIL" not in run.stdout, run.stdout + run.stderr
    return run.stdout


def test_every_cause_voids_exactly_what_depends_on_the_inputs_it_changes(printed):
    fell = {}
    for line in printed.splitlines():
        name, _, rest = line.partition(":")
        if name in CAUSE_INPUTS:
            fell[name] = set(rest.split())
    assert set(fell) == set(CAUSE_INPUTS)
    assert set().union(*fell.values()) <= set(ITEM_INPUTS)
    for cause, changes in CAUSE_INPUTS.items():
        for item, inputs in ITEM_INPUTS.items():
            assert (item in fell[cause]) == bool(inputs & changes), (cause, item)


def test_the_header_declares_the_items_of_this_table_and_no_other(printed):
    header = open(os.path.join(ROOT, "admm-for-rank-based-loss_amd", "csrc", "derived_state.h")).read()
    assert set(re.findall(r"^    bool (\w+) = false;", header, flags=re.M)) == set(ITEM_INPUTS)
    assert set(re.findall(r"^inline void (\w+)\(Derived& s\) \{ s\.changed", header, flags=re.M)) == set(CAUSE_INPUTS)
    assert "#include" not in header        # plain C++: no HIP, nothing else


def test_the_gram_produce_sites(printed):
    assert "gram_formed: local=1 ready=0 eig=0" in printed
    assert "gram_finished: local=1 ready=1 eig=1" in printed


def test_only_the_phases_write_the_flags_directly():
    """the entry points that change an input name a cause; the flags are assigned only where the phases fill and
    consume the buffers (api_iter.hip, api_dist.hip) and behind a group's shared V pass (api_group.hip: v_valid = true)"""
    csrc = os.path.join(ROOT, "admm-for-rank-based-loss_amd", "csrc")
    writes = re.compile(r"der\.(\w+)\s*=(?!=)")
    found = {f: writes.findall(open(os.path.join(csrc, f)).read()) for f in ("api.hip", "api_data.hip", "api_group.hip", "api_kernels.hip")}
    assert found == {"api.hip": [], "api_data.hip": [], "api_group.hip": ["v_valid"], "api_kernels.hip": []}
