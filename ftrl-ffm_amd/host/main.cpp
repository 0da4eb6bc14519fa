// main.cpp -- the trainer CLI (reference src/main.cpp:13-34): parse flags, pick the online or the
// offline task, train.
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <fstream>
#include <stdexcept>
#include <string>

#include "cmd_option.h"
#include "field_ranges.h"
#include "rare_ids.h"
#include "sample_weights.h"
#include "trainer.h"
#include "value_buckets.h"

int main(int argc, char *argv[]) {
  config_options opt;
  try {
    opt.parse_option(argc, argv);
  } catch (const std::invalid_argument &e) {
    std::fprintf(stderr, "invalid argument: %s\n%s", e.what(), std::string(cmd_help).c_str());
    return EXIT_FAILURE;
  }
  try {
    // --model_path is parsed but never used by the reference (cmd_option.cpp:67-68); here a
    // trained model is written there: *.zst -> one zstd frame, anything else -> the text format,
    // and the FTRL accumulators next to it (<path>.nz) so training can resume.
    auto save = [&](ftrl::FtrlModel &m) {
      if (opt.model_path.empty()) return;
      const bool zst = opt.model_path.size() > 4 &&
                       opt.model_path.compare(opt.model_path.size() - 4, 4, ".zst") == 0;
      if (zst) m.save_compressed_model(opt.model_path, 3); else m.save_model(opt.model_path);
      m.save_state(opt.model_path + ".nz");
    };
    // --resume_from / --checkpoint_path: the sparse checkpoint (persist.h) -- the model's changed records
    // and the task's progress, so that a run cut in two gives the files and losses of the run in one piece
    auto run = [&](auto &task) {
      if (!opt.resume_from.empty()) task.restore(task.model_ptr->load_checkpoint(opt.resume_from));
      // --publish_path: the shadow serving engine, brought to a resumed run's epoch by the deltas published so far
      // (a missing or mismatching one ends the run here, before any training)
      if (!opt.publish_path.empty())
        task.model_ptr->prepare_publish(opt.publish_path, opt.publish_weights, task.progress().epochs_done);
      // --apply_deltas PREFIX[:N]: the fresh serving engine takes PREFIX.1.delta .. (every consecutive file that exists,
      // or exactly N of them)
      if (!opt.apply_deltas.empty()) {
        long long features = 0, bytes = 0;
        int applied = 0;
        for (int seq = 1; opt.apply_deltas_n == 0 || seq <= opt.apply_deltas_n; seq++) {
          const std::string file = opt.apply_deltas + "." + std::to_string(seq) + ".delta";
          if (opt.apply_deltas_n == 0 && seq > 1 && !std::ifstream(file).good()) break;
          const ftrl::FtrlModel::DeltaResult r = task.model_ptr->apply_delta(file);
          features += r.n_moved;
          bytes += r.bytes;
          applied++;
        }
        std::printf("applied %d deltas: %lld features, %lld bytes\n", applied, features, bytes);
        ftrl::FtrlModel::TrainProgress behind;  // (one delta per epoch: what is printed is numbered as a checkpoint's would be)
        behind.epochs_done = applied;
        task.restore(behind);
      }
      // --pair_mask @FILE: once, on the model as loaded (the run trains nothing: cmd_option refused --n_epochs > 0)
      if (!opt.pair_mask.empty()) ftrl::load_pair_mask(opt, *task.model_ptr);
      task.train();
      // --auc_key_field on a run that trains nothing (--resume_from ck --n_epochs 0 --eval_data F): one evaluation pass
      // of the loaded model, numbered by the epochs it has behind it -- there is no epoch to print the line after
      // (--field_importance asks for the same one pass: its lines follow an evaluation)
      // (--pair_mask: the masked model's evaluation is what the run is for)
      if ((opt.auc_key_field >= 0 || opt.field_importance || opt.pair_importance || !opt.pair_mask.empty()) && opt.epoch <= 0 && !opt.cmd && !opt.eval_path.empty())
        task.evaluate(static_cast<int>(task.progress().epochs_done));
      task.model_ptr->print_norm_rows();  // (--normalize_rows: one line, after the last epoch or that one evaluation)
      // --field_importance: after the last evaluation, the same model without each field (importance.h);
      // --pair_importance: then the same model without each field pair
      if (opt.field_importance && !opt.cmd) ftrl::run_importance(opt, *task.model_ptr, ftrl::FtrlModel::Ablation::Fields);
      if (opt.pair_importance && !opt.cmd) ftrl::run_importance(opt, *task.model_ptr, ftrl::FtrlModel::Ablation::Pairs);
      // --refresh_weights: every epoch ended with a refresh and nothing has trained since, so the model, the
      // checkpoint and the scores below are those of refreshed weights; a run that trains nothing (--n_epochs 0
      // on a resumed model) refreshes what it loaded here
      if (opt.refresh_weights && (opt.epoch <= 0 || opt.cmd)) ftrl::refresh_and_print(*task.model_ptr, task.progress().epochs_done);
      save(*task.model_ptr);
      if (!opt.checkpoint_path.empty()) task.model_ptr->save_checkpoint(opt.checkpoint_path, 3, task.progress());
      // --predict_data / --predict_out: last, so the scores are those of the model that was written
      if (!opt.predict_path.empty()) {
        const auto t0 = std::chrono::steady_clock::now();
        ftrl::Scorer scorer(opt, &*task.model_ptr);
        const unsigned long long n = scorer.run();
        std::printf("scored %llu rows time: %.4lfs\n", n,
                    std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
      }
      task.model_ptr->print_compact_rows();  // (--compact_rows: one line, last)
    };
    // --pos_weight / --neg_weight / --weight_data: read and checked in full before a model exists
    ftrl::SampleWeights weights = ftrl::load_sample_weights(opt);
    // --field_ranges counted | @FILE, --field_ranges_out: the ranges every model of this run is created with
    // (counted: one pass over the training file, on the device, before a model exists)
    // --min_count T | --rare_ids @FILE, --rare_ids_out: the keep-map every engine of this run folds rare ids by
    // (--min_count: one pass over the training file, on the device, before a model exists) -- ahead of the ranges,
    // which --field_ranges counted then sizes by the ids that stay
    // --bucket_fields LIST | --buckets @FILE, --buckets_out: the bucket table every engine of this run maps numeric
    // fields by (--bucket_fields: one pass over the training file, on the device) -- ahead of both
    ftrl::resolve_value_buckets(opt);
    ftrl::resolve_rare_ids(opt);
    ftrl::resolve_field_ranges(opt);
    if (opt.online) {
      ftrl::FtrlOnline task(opt);
      if (weights.on) task.set_sample_weights(std::move(weights));
      run(task);
    } else {
      ftrl::FtrlOffline task(opt);
      if (weights.on) task.set_sample_weights(std::move(weights));
      run(task);
    }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return EXIT_FAILURE;
  }
  return 0;
}
