// memex::spawn_pretrained(dir, .., kPrecisionCalibrated) on a sentence-transformers directory written by
// tests/test_calibrate_gpu.py: the loader carries "calibrate" through, the embedder opens through mx_encoder_open_calibrated and
// keeps the report.  Prints the report for the Python side to compare with SentenceEmbedder.from_pretrained_dir(precision="auto").
// argv[2] = "load": the loader alone (no GPU).
#include <cstdio>
#include <string>

#include "memex_pretrained.hpp"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    try {
        const memex::PretrainedModel pm = memex::load_pretrained_dir(argv[1], memex::kPrecisionCalibrated);
        if (pm.cfg.precision != memex::kPrecisionCalibrated) {
            std::printf("FAILED the loader resolved precision to %d\n", pm.cfg.precision);
            return 1;
        }
        if (memex::load_pretrained_dir(argv[1]).cfg.precision < 0) {
            std::printf("FAILED the loader's own choice is no mode\n");
            return 1;
        }
        if (argc > 2 && std::string(argv[2]) == "load") {
            std::printf("OK loaded %d\n", pm.cfg.precision);
            return 0;
        }
        auto [th, emb] = memex::spawn_pretrained(argv[1], memex::ModelConfig{}, 0, memex::kPrecisionCalibrated);
        const mx_encoder_calibration *r = emb->calibration();
        if (!r) {
            std::printf("FAILED no report\n");
            return 1;
        }
        const auto one = emb->encode_single("the state of the union");
        std::printf("OK %d %d %d %d %.17g %zu", r->chosen, r->tried, r->probe_seqs, r->probe_tokens, r->bar, one ? one->vector.size() : (size_t)0);
        for (int m = 0; m < 4; ++m) std::printf(" %.17g", r->pair_dev[m]);
        std::printf("\n");
        emb->shutdown();
        th.join();
        return 0;
    } catch (const memex::EmbeddingError &e) {
        std::printf("REFUSED %s\n", e.what());
        return 3;
    }
}
