"""tests/cpp/harness.cpp keeps up with include/apd.hpp, no GPU: every apd_* function the header calls belongs to a wrapper in the
table below, and the harness source calls every wrapper of the table by name.  A wrapper added to the header without a harness mode
is a symbol this table does not know; a call dropped from the harness is a pattern that no longer matches.  What the modes print is
compared with the checkers by tests/test_gpu_cpp_mirror.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# wrapper of apd.hpp -> (how the harness calls it, the C functions it reaches)
WRAPPERS = {
    "check": (r"apd::check\(", ["apd_status_string", "apd_last_error"]),
    "Context": (r"apd::Context \w+\(", ["apd_create", "apd_destroy"]),
    "Context::set_distance_mode": (r"\.set_distance_mode\(", ["apd_set_distance_mode"]),
    "AutoEncoder::from_file": (r"apd::AutoEncoder::from_file\(", ["apd_autoencoder_parse", "apd_autoencoder_copy"]),
    "AutoEncoder::save_file": (r"\.save_file\(", ["apd_autoencoder_serialize"]),
    "AutoEncoder::encoded": (r"\.encoded\(", ["apd_encode"]),
    "Discovery::from_toml": (r"apd::Discovery::from_toml\(", ["apd_discovery_parse_toml"]),
    "Discovery::alignment_params": (r"\.alignment_params\(", ["apd_discovery_alignment_params"]),
    "Alignment::construct_alignment": (r"\.construct_alignment\(", ["apd_align_pair"]),
    "Alignment::construct_alignment(with_path)": (r"\.construct_alignment\([^;]*, true\);", ["apd_path_bound", "apd_align_pair_path"]),
    "Alignment::path": (r"\.path\(\)", []),
    "Alignment::score": (r"\.score\(\)", []),
    "Batch::join": (r"apd::Batch::join\(", ["apd_batch_join", "apd_batch_destroy"]),
    "Batch::len": (r"\bjoined\.len\(\)", ["apd_batch_len"]),
    "Batch::first_len": (r"\.first_len\(\)", ["apd_batch_first_len"]),
    "AlignmentWorkers": (r"apd::AlignmentWorkers \w+\(", ["apd_batch_create", "apd_batch_destroy", "apd_multi_destroy"]),
    "AlignmentWorkers::align_all": (r"\.align_all\(\w+(\.\w+)?\)", ["apd_align_all"]),
    "AlignmentWorkers::align_all(devices)": (r"\.align_all\(\w+, std::vector<int>", ["apd_multi_create", "apd_multi_batch_create", "apd_multi_align_all",
                                                                                  "apd_multi_ranks_seen", "apd_multi_last_error", "apd_multi_destroy"]),
    "AlignmentWorkers::collective": (r"\.collective\(\)", ["apd_multi_collective"]),
    "AlignmentWorkers::cross": (r"\.cross\(", ["apd_align_cross"]),
    "AlignmentWorkers::spot": (r"\.spot\(", ["apd_spot"]),
    "AlignmentWorkers::spot(streams)": (r"\.spot\([^;]*&second\)", ["apd_spot"]),
    "spot_hits": (r"apd::spot_hits\(", ["apd_spot_hits"]),
    "AlignmentWorkers::spot_paths": (r"\.spot_paths\(", ["apd_spot_paths"]),
    "AlignmentWorkers::spot_paths(streams)": (r"\.spot_paths\([^;]*&second\)", ["apd_spot_paths"]),
    "AlignmentWorkers::spot_stream": (r"\.spot_stream\(", ["apd_spot_stream_create", "apd_spot_stream_destroy"]),
    "SpotStream(SpotStream &&)": (r"apd::SpotStream \w+\(std::move\(\w+\)\)", []),
    "SpotStream::push": (r"\bstream\.push\(", ["apd_spot_stream_push"]),
    "SpotStream::reset": (r"\bstream\.reset\(", ["apd_spot_stream_reset"]),
    "SpotStream::columns": (r"\bstream\.columns\(", ["apd_spot_stream_columns"]),
    "SpotStream::keep": (r"\bstream\.keep\(", ["apd_spot_stream_keep"]),
    "SpotStream::history": (r"\bstream\.history\(", ["apd_spot_stream_history"]),
    "SpotStream::paths": (r"\bstream\.paths\(", ["apd_spot_stream_paths"]),
    "AlignmentWorkers::barycenters": (r"\.barycenters\(", ["apd_barycenters"]),
    "AgglomerativeClustering::clustering": (r"apd::AgglomerativeClustering::clustering\(", ["apd_clustering"]),
    "AgglomerativeClustering::cluster_sets": (r"apd::AgglomerativeClustering::cluster_sets\(", ["apd_cluster_sets"]),
    "AgglomerativeClustering::cross_linkage": (r"apd::AgglomerativeClustering::cross_linkage\(", ["apd_cross_linkage"]),
    "AgglomerativeClustering::medoids": (r"apd::AgglomerativeClustering::medoids\(", ["apd_cluster_medoids"]),
    "dendrograms": (r"apd::dendrograms\(", ["apd_dendrograms"]),
}


def code_of(path):
    """The file without its comments."""
    with open(path) as fp:
        text = fp.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def header_calls():
    return set(re.findall(r"\b(apd_[a-z0-9_]+)\s*\(", code_of(os.path.join(ROOT, "include", "apd.hpp"))))


def unnamed_wrappers(harness_code, wrappers=WRAPPERS):
    return sorted(name for name, (pattern, _) in wrappers.items() if not re.search(pattern, harness_code))


def test_every_function_the_header_calls_belongs_to_a_wrapper_of_the_table():
    called = header_calls()
    assert len(called) >= 40, called                                             # the parse found the header's calls at all
    known = {symbol for _, symbols in WRAPPERS.values() for symbol in symbols}
    assert called - known == set(), "apd.hpp calls functions no wrapper of the table reaches: add the wrapper here and a harness mode"
    assert known - called == set(), "the table names functions apd.hpp no longer calls"


def test_the_harness_calls_every_wrapper_by_name():
    harness = code_of(os.path.join(ROOT, "tests", "cpp", "harness.cpp"))
    assert unnamed_wrappers(harness) == []


def test_a_wrapper_dropped_from_the_harness_is_noticed():
    harness = code_of(os.path.join(ROOT, "tests", "cpp", "harness.cpp"))
    for name, gone in (("AlignmentWorkers::spot_paths", ".spot_paths("), ("SpotStream::keep", "stream.keep("),
                       ("AgglomerativeClustering::medoids", "AgglomerativeClustering::medoids("), ("Batch::join", "Batch::join(")):
        assert gone in harness
        assert name in unnamed_wrappers(harness.replace(gone, ".something_else(")), name
    spoken_of = harness.replace("stream.keep(", "x(") + "\n// stream.keep(history): a comment is no call\n"
    assert "SpotStream::keep" in unnamed_wrappers(re.sub(r"//[^\n]*", "", spoken_of))
