// tests/cpp/test_policy_rows.cpp — HipTDTCompressionProtocol::should_transform (GPU codec context)
// answers what the reference did on the equality rows of the routing record: width 4, the `mt`,
// `n64`, `bw` and `cpu` cases that sit on an equality (min_tensor_size, the 64-byte floor, both
// thresholds).  Built like tests/cpp/test_substrate.cpp (psyne_amd/build.py), driven by
// tests/test_gpu_policy_matrix.py.  Prints "cpp policy rows OK" on success.
#include <psyne_amd/hip_tdt_protocol.hpp>

#include <cstdio>
#include <vector>

using namespace psyne_amd;

// Rows of tests/golden/policy_matrix.json (field `st`) with their cases' settings from
// tests/policy_cases.py.  Regenerate from the JSON when tests/golden/make_policy_matrix.py rewrites it.
struct PolicyRow {
    const char *name;
    size_t n, min_tensor;
    double bandwidth, cpu, bandwidth_threshold, cpu_threshold;
    bool verdict;
};
static const PolicyRow kPolicyRows[] = {
    {"ws4_mt_mt1024_n1020_off", 1020, 1024, 10, 0.5, 100, 0.80000000000000004, false},
    {"ws4_mt_mt1024_n1024_on", 1024, 1024, 10, 0.5, 100, 0.80000000000000004, true},
    {"ws4_mt_mt4112_n4108_off", 4108, 4112, 10, 0.5, 100, 0.80000000000000004, false},
    {"ws4_mt_mt4112_n4112_on", 4112, 4112, 10, 0.5, 100, 0.80000000000000004, true},
    {"ws4_mt_mt65552_n65548_off", 65548, 65552, 10, 0.5, 100, 0.80000000000000004, false},
    {"ws4_mt_mt65552_n65552_on", 65552, 65552, 10, 0.5, 100, 0.80000000000000004, true},
    {"ws4_n64_mt0_n60_off", 60, 0, 10, 0.5, 100, 0.80000000000000004, false},
    {"ws4_n64_mt0_n64_on", 64, 0, 10, 0.5, 100, 0.80000000000000004, true},
    {"ws4_bw_t100_b100.0_n4096_off", 4096, 1024, 100, 0.5, 100, 0.80000000000000004, false},
    {"ws4_bw_t100_b99.99999999999999_n4096_on", 4096, 1024, 99.999999999999986, 0.5, 100, 0.80000000000000004, true},
    {"ws4_bw_t50_b50.0_n4096_off", 4096, 1024, 50, 0.5, 50, 0.80000000000000004, false},
    {"ws4_bw_t50_b75.0_n4096_off", 4096, 1024, 75, 0.5, 50, 0.80000000000000004, false},
    {"ws4_cpu_t0.8_c0.8_n4096_on", 4096, 1024, 10, 0.80000000000000004, 100, 0.80000000000000004, true},
    {"ws4_cpu_t0.8_c0.8000000000000002_n4096_off", 4096, 1024, 10, 0.80000000000000016, 100, 0.80000000000000004, false},
    {"ws4_cpu_t0.25_c0.25_n4096_on", 4096, 1024, 10, 0.25, 100, 0.25, true},
    {"ws4_cpu_t0.25_c0.3_n4096_off", 4096, 1024, 10, 0.29999999999999999, 100, 0.25, false},
};

int main() {
    std::vector<uint8_t> data(65552, 0);
    for (const PolicyRow &r : kPolicyRows) {
        TDTConfig cfg;
        cfg.sample_fraction = 1.0f;
        cfg.min_tensor_size = r.min_tensor;
        cfg.bandwidth_threshold_mbps = r.bandwidth_threshold;
        cfg.cpu_usage_threshold = r.cpu_threshold;
        HipTDTCompressionProtocol p(cfg);
        p.update_network_metrics(r.bandwidth, 1.0);
        p.update_system_metrics(r.cpu);
        if (p.should_transform(data.data(), r.n) != r.verdict) {
            std::printf("FAILED: row %s: should_transform is %d\n", r.name, r.verdict ? 0 : 1);
            return 1;
        }
    }
    std::printf("cpp policy rows OK rows=%zu\n", sizeof(kPolicyRows) / sizeof(kPolicyRows[0]));
    return 0;
}
