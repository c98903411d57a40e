"""CPU: the C-ABI library loads and exports every symbol include/vq_amd.h declares (no compute calls)."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    with open(os.path.join(ROOT, "include", "vq_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(vq_\w+)\s*\(", text, flags=re.M)))


def test_header_declares_entry_points():
    names = _declared()
    assert len(names) >= 102
    for must in ("vq_db_create", "vq_db_scan", "vq_db_select", "vq_db_topk", "vq_tsn_create", "vq_tsn_forward", "vq_flow_tvl1", "vq_flow_tile_cut"):
        assert must in names


def test_library_exports_every_declared_symbol():
    import video_query_algorithms_amd as vqa
    lib = vqa.load_library()
    raw = ctypes.CDLL(vqa._lib.LIB_PATH)
    for name in _declared():
        assert hasattr(raw, name), "libvqamd.so does not export %s" % name
    assert lib.vq_abi_version() == vqa._lib.ABI_VERSION == 12


def test_ctypes_table_covers_the_header():
    import video_query_algorithms_amd as vqa
    assert sorted(vqa._lib.exported_symbols()) == _declared()
    assert len(vqa._lib.exported_symbols()) == 102                       # ABI 12: 101 of ABI 11 + vq_flow_tile_cut
    with open(os.path.join(ROOT, "include", "vq_amd.h")) as f:
        proto = re.search(r"int\s+vq_flow_tile_cut\s*\(([^)]*)\)", f.read()).group(1)
    assert [a.split()[0] for a in proto.split(",")] == ["vq_flow*", "int32_t", "int32_t", "int32_t"]      # handle, level, n_pairs, out[6]
    assert len(vqa._lib.SIGNATURES["vq_flow_tile_cut"]) == 4


def test_header_is_plain_c():
    """The boundary must be consumable from C (cgo / JNI / ctypes): compile the header with gcc -std=c99."""
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "vq_amd.h"\nint main(void){ vq_layer_desc l; (void)l; return VQ_OK; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


def test_no_product_import_of_the_oracle():
    """The shipped package must never route through oracle/ (or any CPU fallback)."""
    pkg = os.path.join(ROOT, "video-query-algorithms_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".cpp")):
                with open(os.path.join(dirpath, fn)) as f:
                    text = f.read()
                assert not re.search(r"^\s*(from|import)\s+(oracle|sim_oracle|tsn_oracle)\b", text, flags=re.M), fn


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    import video_query_algorithms_amd as vqa
    monkeypatch.setattr(vqa._lib, "_lib", None)
    monkeypatch.setenv("VQ_AMD_LIB", str(tmp_path / "nope.so"))
    with pytest.raises(ImportError):
        vqa._lib.load()
    monkeypatch.delenv("VQ_AMD_LIB")
    monkeypatch.setattr(vqa._lib, "_lib", None)
    vqa._lib.load()


def test_install_patches_exactly_the_hot_path_methods():
    """install() swaps the four Ticket methods and optimize_weights on the classes it is given, and leaves every other method
    alone -- checked on look-alikes that carry every method name of the reference's own Ticket and Hyperparameter classes."""
    import video_query_algorithms_amd as vqa
    ticket_methods = ["__init__", "add_matches_to_database", "add_note", "catch_errors", "change_process_state", "compute_similarities",
                      "compute_scores", "create_final_report", "create_match", "create_query_result", "lowest_scoring_user_match",
                      "select_clips_to_review", "_get_candidate_features", "_request", "_post_file"]
    hp_methods = ["__init__", "optimize_weights", "fine_tune", "_quad_fit"]
    grafted = ("compute_similarities", "compute_scores", "select_clips_to_review", "lowest_scoring_user_match")

    def own(name):
        def method(self, *a, **kw):
            return name
        return method
    Ticket = type("Ticket", (), {n: own(n) for n in ticket_methods})
    Hp = type("Hyperparameter", (), {n: own(n) for n in hp_methods})
    untouched = [n for n in ticket_methods if n not in grafted]
    hp_untouched = [n for n in hp_methods if n != "optimize_weights"]
    before = {n: getattr(Ticket, n) for n in untouched}
    hp_before = {n: getattr(Hp, n) for n in hp_untouched}
    vqa.install(Ticket, Hp)
    for n in grafted:
        assert getattr(Ticket, n) is getattr(vqa.TicketScoring, n)
    assert Hp.optimize_weights is vqa.Hyperparameter.optimize_weights
    for n in untouched:
        assert getattr(Ticket, n) is before[n]
    for n in hp_untouched:
        assert getattr(Hp, n) is hp_before[n]
    assert Ticket.feature_db is None


def test_comm_group_without_rccl_reports_unsupported(tmp_path):
    """A host without librccl (VQ_RCCL_LIB names the only candidate; here a file that does not exist): every vq_comm_* entry
    point returns VQ_E_UNSUPPORTED with the loader's message -- no crash inside the library, no HIP call."""
    import subprocess
    code = (
        "import ctypes as C, sys\n"
        "sys.path.insert(0, %r)\n"
        "from video_query_algorithms_amd import _lib\n"
        "lib = _lib.load()\n"
        "buf = C.create_string_buffer(128)\n"
        "rc = lib.vq_comm_unique_id(buf)\n"
        "msg = lib.vq_last_error().decode()\n"
        "assert rc == -5, (rc, msg)\n"
        "assert 'librccl not found' in msg and 'no_such_rccl' in msg, msg\n"
        "h = C.c_void_p()\n"
        "assert lib.vq_comm_init(0, 1, buf, 0, C.byref(h)) == -5\n"
        "print('ok')\n" % ROOT)
    env = dict(os.environ, VQ_RCCL_LIB=str(tmp_path / "no_such_rccl.so"))
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout


def test_every_environment_switch_is_listed_in_the_header():
    """include/vq_amd.h documents ALL switches: every VQ_* variable the library (getenv) or the package (os.environ) reads appears there."""
    import glob
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "vq_amd.h")).read()
    names = set()
    pkg = os.path.join(root, "video-query-algorithms_amd")
    for path in glob.glob(os.path.join(pkg, "**", "*"), recursive=True):
        if not path.endswith((".py", ".hip", ".cc", ".h")):
            continue
        text = open(path, errors="replace").read()
        for m in re.finditer(r'getenv\("(VQ_[A-Z0-9_]+)"\)|environ(?:\.get|\.setdefault)?\(?\[?"(VQ_[A-Z0-9_]+)"', text):
            names.add(m.group(1) or m.group(2))
    assert len(names) > 20
    missing = sorted(n for n in names if n not in header and not n.startswith("VQ_FANOUT_"))
    assert "VQ_FANOUT_*" in header and not missing, missing
