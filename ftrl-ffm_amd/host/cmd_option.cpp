#include "cmd_option.h"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <vector>

const std::string_view cmd_help =
    "\nUsage: ./ftrl_ffm_main [<options>]\n\noptions:\n"
    "--model_path <model_path>: set the output model path\n"
    "--train_data <data_path>: set the train data path\n"
    "--eval_data <data_path>: set the eval data path\n"
    "--model_type <model_type>: LR, FM or FFM\n"
    "--init_mean <mean>: mean for parameter initialization\tdefault:0.0\n"
    "--init_stddev <stddev>: stddev for parameter initialization\tdefault:0.02\n"
    "--n_fields <n_fields>: number of fields in FFM\tdefault:8\n"
    "--n_feats <n_feats>: number of total features\tdefault:10000\n"
    "--n_factors <n_factors>: number of embed size in FM and FFM\tdefault:16\n"
    "--w_alpha <w_alpha>: alpha is one of the learning rate parameters\tdefault:1e-4\n"
    "--w_beta <w_beta>: beta is one of the learning rate parameters\tdefault:1.0\n"
    "--w_l1 <w_L1_reg>: L1 regularization parameter of w\tdefault:0.1\n"
    "--w_l2 <w_L2_reg>: L2 regularization parameter of w\tdefault:5.0\n"
    "--n_threads <threads_num>: host threads for parsing\tdefault:1\n"
    "--n_epochs <epochs>: how many epochs to train; with --resume_from: how many MORE; 0 trains nothing\n"
    "              (--resume_from ck --n_epochs 0 --predict_data F --predict_out P scores a saved model;\n"
    "              --train_data may then be left out)\tdefault:1\n"
    "--online <online>: whether to online training mode\tdefault:true\n"
    "--batch_size <rows>: rows per block sent to the GPU\tdefault:4096\n"
    "--batch_ramp <r>: block size grows as rows_seen/r (0 disables)\tdefault: by w_alpha (32 up to 1e-3)\n"
    "--seed <seed>: seed of the weight init and the offline shuffle\tdefault:42\n"
    "--device <id>: HIP device ordinal\tdefault:0\n"
    "--n_gpus <n>: shard the field pairs over n devices (one engine each, RCCL all-reduce of the\n"
    "              partial logits per block)\tdefault:1\n"
    "--field_ranges <uniform|none|counted|@FILE>: uniform = field f owns ids [f*n_feats/n_fields, (f+1)*n_feats/n_fields),\n"
    "              shards then store only their own slots.  counted (FFM, one GPU) = before a model exists --train_data is\n"
    "              streamed once and the distinct ids of every field are counted on the device (a HyperLogLog sketch per\n"
    "              field, +-0.8 %); every field then owns a share of n_feats in proportion to its count, above a floor of\n"
    "              min(4096, n_feats/(2*n_fields)) ids.  Prints one `field f: ~D distinct ids, ids [lo, hi)` per field and\n"
    "              `field ranges: counted from R rows (E entries, B erased) in T s; ~S distinct ids for N features (load X)`:\n"
    "              a load above 1 means collisions, raise --n_feats.  @FILE = the ranges of such a run, read from FILE:\n"
    "              n_fields + 1 ascending integers, one per line, from 0 to n_feats.  Both are honoured wherever uniform is\n"
    "              on one GPU: they shape the id mapping under --hash_feats and are a hint to the grouping otherwise.  The\n"
    "              ranges are not recorded in checkpoints: counted is refused with --resume_from, a resumed or scoring run\n"
    "              passes @FILE.  --n_gpus > 1 takes uniform only\tdefault:none\n"
    "--field_ranges_out <path>: write the ranges in use (uniform, counted or @FILE) to path, one integer per line\n"
    "--checkpoint_path <path>: after training, write a sparse resumable checkpoint: only the features that\n"
    "              differ from a fresh model of this seed (found by a device scan), with w, n, z, the bias and the\n"
    "              trainer's progress (one GPU only)\n"
    "--resume_from <path>: load such a checkpoint before training; needs the same model shape, --seed,\n"
    "              --init_mean, --init_stddev, --learn and --hash_feats (checked); the FTRL hyper-parameters (--w_alpha,\n"
    "              --w_beta, --w_l1, --w_l2), --batch_size and --batch_ramp are NOT recorded in the file: pass the same ones\n"
    "              and the resumed run continues the interrupted one bit for bit.  Under --hash_feats, --field_ranges\n"
    "              shapes the id mapping and is not recorded either: a resumed run must pass the same value\n"
    "--metrics <auc|none>: auc = after each epoch's loss line one more line with the AUC of the same rows -- training:\n"
    "              of the pre-update predictions (progressive validation) --, histogrammed on the device in 2^20\n"
    "              score bins; the +- is the most the exact rank AUC can differ\tdefault:none\n"
    "--auc_key_field <F>: with --metrics auc, after each AUC line one more with the grouped AUC (GAUC): the AUC inside\n"
    "              each value of field F (the first entry of field F in a row is its key: a user, a request, a placement),\n"
    "              averaged over the keys that hold both classes, weighted by their rows; sorted and ranked on the device\n"
    "              in exact integers.  Prints `epoch N <train|eval> gauc: G (K keys, M mixed, R of T rows; U unkeyed,\n"
    "              O over capacity, X nan)`: R rows of the M keys with both classes, of T rows kept.  FFM only, one GPU.\n"
    "              With --resume_from ck --n_epochs 0 --eval_data F (and --serve_weights or not) the loaded model is\n"
    "              evaluated once, numbered by the epochs it has behind it\n"
    "--auc_key_rows <N>: rows kept per pass for it (8 bytes each, twice, in HBM); the rest count as over capacity\tdefault:16777216\n"
    "--predict_data <data_path>: after training (and after the model / checkpoint is written) score this file:\n"
    "              one prediction per row, in file order; its label column is parsed and ignored\n"
    "--predict_out <path>: where the predictions go, one per line, each the shortest decimal that parses back\n"
    "              to the same float (nan, inf, -inf by name); needs --predict_data and the other way round.\n"
    "              Prints `scored N rows time: Ts`.  With --n_gpus > 1 the blocks are predicted one by one\n"
    "              (the synchronous group call), on one GPU they stream through the pipelined prediction\n"
    "--predict_output <prob|logit>: what is written\tdefault:prob\n"
    "--pos_weight <P> / --neg_weight <N>: weight of every positive / negative training row: finite, >= 0.  The\n"
    "              row's gradient is scaled by it (the correction for down-sampled negatives)\tdefault:1\n"
    "--weight_data <path>: one decimal weight per line, as many lines as --train_data has rows; a row's weight is\n"
    "              the float product of its line and its class weight; the file is checked in full before a model exists, for\n"
    "              which --train_data is read once more to count its rows.  With any of the three flags the `train loss`\n"
    "              line is sum(w * loss) / sum(w); eval loss, AUC lines and predictions stay unweighted.  Weights are\n"
    "              not saved with the model or the checkpoint: a run resumed with --resume_from needs the same flags\n"
    "--learn <bool>: keep initial latent weights until their first gradient and use g2*g2 at\n"
    "                ffm.cpp:118, so FM/FFM factors train (NOT the reference's results)\tdefault:false\n"
    "--refresh_weights <bool>: training refreshes a weight from its accumulators only BEFORE it updates them, so what\n"
    "              evaluation, --model_path, --checkpoint_path and --predict_data read is one update behind: a feature\n"
    "              seen in one block only is scored as if never seen.  true = one pass over the model sets every stored\n"
    "              w = W(n, z) where (n, z) are not both zero bits (under --learn a latent slot whose n is not > 0 keeps\n"
    "              its w) after each epoch's training and before its evaluation, before the model and the checkpoint are\n"
    "              written and before --predict_data is scored (also with --resume_from ck --n_epochs 0), and prints\n"
    "              `epoch N weights: linear L live, Z nonzero, M moved; latent L live, Z nonzero, M moved`.  (n, z) and\n"
    "              the `train loss` lines do not change by a bit\tdefault:false\n"
    "--hash_feats <bool>: the hashing trick, on the device: every non-negative id of the data, of any size, is hashed\n"
    "              into the model's id space instead of being dropped when it is >= n_feats, salted by its field -- into\n"
    "              [0, n_feats) with --field_ranges none, into its field's own range with uniform, which lets --n_gpus N\n"
    "              train any libffm file and gives one GPU the per-field sort and the regular-block forms; LR / FM hash\n"
    "              libsvm ids into [0, n_feats).  Negative ids (FFM: and fields outside [0, n_fields)) stay dropped.  The\n"
    "              model, the checkpoint and every id printed are hashed ids; --n_feats bounds the model, not the data\tdefault:false\n"
    "--serve_weights <none|f32|f16>: score a saved model from a serving engine, which holds the weights alone (no n, z):\n"
    "              f32 = the same fp32 bits in a third of the memory, the same predictions bit for bit; f16 = IEEE half\n"
    "              precision (round to nearest even) in a sixth of the memory, half the bytes read per prediction.  Only\n"
    "              with --resume_from ck --n_epochs 0 (then --predict_data / --predict_out, --predict_output, --metrics auc\n"
    "              and --hash_feats as always); FFM only, one GPU, rows of at most 128 entries, no training: refused with\n"
    "              --n_epochs > 0, --model_path, --checkpoint_path, --n_gpus > 1 and --refresh_weights true (write the\n"
    "              checkpoint with --refresh_weights true instead).  Prints `serving weights: <fmt>, <bytes> bytes of model`\tdefault:none\n"
    "--compact_rows <bool>: a block whose values are all 1 (what a categorical libffm file is after --hash_feats) goes\n"
    "              to the GPU without its value array, and an FFM block whose rows are one entry per field in field order\n"
    "              without its field array: the device writes both itself, a third of the block's bytes over PCIe each.\n"
    "              Noted per row while the file is parsed; training, evaluation, --predict_data and --serve_weights.  Losses,\n"
    "              AUC lines, scores, model files and checkpoints do not change by a bit.  Prints\n"
    "              `compact rows: V of B blocks without values, F without fields`\tdefault:false\n"
    "--field_importance <bool>: which fields earn their place?  true = after the last epoch's evaluation (with\n"
    "              --resume_from ck --n_epochs 0 --eval_data F, and --serve_weights or not: after the one evaluation of the\n"
    "              loaded model) --eval_data is streamed once more and every row is predicted n_fields + 1 ways in one pass\n"
    "              on the device: as it is, and without each field (every entry of the field removed; exact, not an\n"
    "              approximation).  Prints `field importance: R rows, loss L, auc A`, then per field, in field order,\n"
    "              `field f: without it loss L (delta D), auc A (delta D)`; the AUC parts only with --metrics auc.  Needs\n"
    "              --eval_data; FFM only, one GPU, --n_fields <= 64, --n_factors 4, 8, 16, 32 or 64, rows of at most 128\n"
    "              entries.  Nothing else of the output changes\tdefault:false\n"
    "--pair_importance <bool>: which interactions carry the model?  true = one more pass over --eval_data after the last\n"
    "              evaluation (after --field_importance's when both are given; with --resume_from ck --n_epochs 0 as that\n"
    "              flag, --serve_weights or not): every row is predicted n_fields (n_fields + 1) / 2 + 1 ways in one pass\n"
    "              on the device: as it is, and without the terms between fields f and g for every pair f <= g (f = g:\n"
    "              between two entries of one field; linear terms stay; exact, not an approximation).  Prints `pair\n"
    "              importance: R rows, loss L, auc A`, then `pair f g: without it loss L (delta D), auc A (delta D)` per\n"
    "              pair whose loss sum differs from the whole row's, in index order, then `pair importance: P of V pairs\n"
    "              listed, Q never changed a row`; the AUC parts only with --metrics auc, which keeps a 16.8 MB histogram\n"
    "              per pair on the device (13 GB at 39 fields, 35 GB at 64; printed before it is allocated).  Reads through\n"
    "              the host parser.  Needs --eval_data; FFM only, one GPU, --n_fields <= 64, --n_factors 4, 8, 16, 32 or\n"
    "              64, rows of at most 128 entries.  Nothing else of the output changes\tdefault:false\n"
    "--pair_keep <N> --pair_mask_out <file>: with --pair_importance true: rank all V pairs by delta = loss without the pair\n"
    "              minus loss of the rows (largest first, ties to the lower pair index), keep the first N (0 <= N <= V) and\n"
    "              write them as a mask file: `ffm-pair-mask 1 <n_fields> <n_kept>`, then one `f g` line per kept pair.\n"
    "              Prints `pair mask: kept N of V pairs, smallest kept delta D -> FILE`; a delta that is not finite ends the\n"
    "              run.  Both flags go together\tdefault:(none)\n"
    "--pair_curve <LIST|auto>: with --pair_importance true: where does pruning start to hurt?  After the pairs' pass, rank\n"
    "              the pairs as --pair_keep does and make one more pass over --eval_data that predicts every row under\n"
    "              `keep the best N pairs` for every listed N at once, on the device, exactly.  LIST is 1 to 64\n"
    "              comma-separated N in [0, V]; auto is round(i V / 63) for i = 0 .. 63.  Prints `pair curve: R rows, loss L,\n"
    "              auc A`, then, ascending in N, `keep N of V pairs: loss L (delta D), auc A (delta D)`; the AUC parts\n"
    "              only with --metrics auc (a 16.8 MB histogram per listed N)\tdefault:(none)\n"
    "--pair_loss_budget <T>: with --pair_curve and --pair_mask_out <file>, in place of --pair_keep: write the mask of the\n"
    "              smallest listed N whose per-row loss delta is <= T.  Prints `pair mask: kept N of V pairs, loss delta D\n"
    "              within budget T -> FILE`; if no listed N meets the budget nothing is written, a line says so and the\n"
    "              run exits non-zero\tdefault:(none)\n"
    "--pair_mask <@file>: a run that trains nothing (--n_epochs 0 with --resume_from ck, --serve_weights or not, or with\n"
    "              --apply_deltas) predicts with the file's pairs only: the terms of every other pair are left out, and\n"
    "              their gathers are not made.  --eval_data, --metrics auc, --auc_key_field, --predict_data / --predict_out\n"
    "              and --device_rows true then give the masked model's numbers.  Prints `pair mask: K of V pairs kept, from\n"
    "              FILE`.  FFM only, one GPU, --n_fields <= 64, --n_factors 4, 8, 16, 32 or 64; not with --n_epochs > 0,\n"
    "              --field_importance, --pair_importance or --cmd true\tdefault:(none)\n"
    "--publish_path <prefix>: after every epoch's training (after that epoch's --refresh_weights refresh when it is on,\n"
    "              before its evaluation) write <prefix>.<epochs_done>.delta: the features whose serving bits moved since\n"
    "              the previous delta, in a serving engine's own format -- delta 1 is relative to a fresh serving engine of\n"
    "              the same --seed and init.  A shadow serving engine on the same GPU does the comparing: it costs a third\n"
    "              (f32) or a sixth (f16) of the training engine's memory on top of it.  Prints `epoch N published: M of F\n"
    "              features moved, B bytes -> FILE`.  With --resume_from ck the shadow first applies <prefix>.1 ..\n"
    "              <prefix>.<epochs of ck>; a missing or mismatching file is an error before any training.  FFM only, one\n"
    "              GPU, --n_factors 4, 8, 16, 32 or 64; not with --cmd true or --serve_weights\tdefault:(none)\n"
    "--publish_weights <f32|f16>: the format of the deltas --publish_path writes\tdefault:f32\n"
    "--apply_deltas <prefix[:N]>: with --serve_weights <fmt> --n_epochs 0: a fresh serving engine takes <prefix>.1.delta,\n"
    "              <prefix>.2.delta .. up to N (default: every consecutive file that exists; at least one must), prints\n"
    "              `applied D deltas: M features, B bytes`, then evaluates or scores as --resume_from ck --n_epochs 0 does.\n"
    "              Not with --resume_from, --n_epochs > 0 or a --serve_weights other than the files' format\tdefault:(none)\n"
    "--min_count <T>: ids seen fewer than T times in --train_data share one \"rare\" id per field (libffm's Criteo recipe\n"
    "              used 10).  --train_data is streamed once before a model exists and the device counts every id's hashed\n"
    "              slot up to T; with --field_ranges counted it is then streamed a second time so that the ranges are sized\n"
    "              by the ids that stay.  From then on every id whose slot was seen fewer than T times is replaced by\n"
    "              2147483647 before it is hashed: training, evaluation, --predict_data, --serve_weights, --field_importance\n"
    "              and --publish_path alike.  Prints `rare ids: counted R rows (E entries, X erased) in S s; K of 2^B slots\n"
    "              kept at min_count T, F entries folded`.  Needs --hash_feats true and --train_data; one GPU; not with\n"
    "              --resume_from or --rare_ids (a saved model takes its map from --rare_ids @FILE: it is not in the\n"
    "              checkpoint).  0 and 1 are off\tdefault:0\n"
    "--rare_bits <B>: the counter of --min_count has 2^B slots (ids that share a slot are counted together), 8 .. 30\n"
    "              \tdefault:the smallest B with 2^B >= 4 * n_feats, at least 16 and at most 30\n"
    "--rare_ids_out <file>: write the keep-map of --min_count (or of --rare_ids @FILE) there\tdefault:(none)\n"
    "--rare_ids <@file>: fold by the keep-map an earlier run wrote with --rare_ids_out instead of counting one; the run\n"
    "              goes on exactly as the counting run did.  Needs --hash_feats true; one GPU\tdefault:(none)\n"
    "--bucket_fields <list>: numeric fields, such as 0-12,20, whose entries field:id:value become field:bucket:1 with\n"
    "              quantile buckets of the value.  --train_data is streamed once before a model exists (ahead of the\n"
    "              --min_count and --field_ranges counted passes) and the device counts a histogram of 65536 value bins per\n"
    "              field; the host cuts each into --n_buckets buckets of equal mass.  Prints `field f: N values in D bins ->\n"
    "              K buckets` per field and `value buckets: counted R rows (E entries, X nan) in S s`.  A bucketed entry is\n"
    "              never folded by --min_count; --field_ranges counted takes such a field's count as its edges + 2.  Needs\n"
    "              --hash_feats true, an FFM model and --train_data; one GPU; not with --resume_from or --buckets (a saved\n"
    "              model takes its table from --buckets @FILE: it is not in the checkpoint)\tdefault:(none)\n"
    "--n_buckets <B>: buckets per field of --bucket_fields, 2 .. 256\tdefault:32\n"
    "--buckets_out <file>: write the bucket table of --bucket_fields (or of --buckets @FILE) there\tdefault:(none)\n"
    "--buckets <@file>: bucket by the table an earlier run wrote with --buckets_out instead of counting one; the run goes\n"
    "              on exactly as the counting run did.  Needs --hash_feats true and an FFM model; one GPU\tdefault:(none)\n"
    "--normalize_rows <bool>: instance-wise normalisation, on the device: every row's values are divided by the row's\n"
    "              Euclidean length, sqrt(sum v^2) over the entries the model keeps, before anything reads them (libffm and\n"
    "              xLearn do this by default, so their --w_alpha / --w_beta / L1 / L2 carry over); after --hash_feats,\n"
    "              --min_count and --bucket_fields, a bucketed entry counting as the 1 it became.  A row whose length is zero\n"
    "              or not finite stays as it came.  Training, evaluation, --predict_data, --serve_weights and\n"
    "              --field_importance alike (which drops a field after normalising).  Prints `normalized rows: R scaled, U\n"
    "              left as they came (zero or non-finite norm)`.  The checkpoint records the setting and --resume_from\n"
    "              refuses the other one; model files and serving deltas do not: a run that scores or serves such a model\n"
    "              passes the flag again, as it passes --field_ranges @FILE.  One GPU\tdefault:false\n"
    "--device_parse <bool>: the counting passes over --train_data (--bucket_fields, --min_count, --field_ranges counted)\n"
    "              read the file as raw bytes and the device parses them: plain ids of at most 9 digits and plain decimals\n"
    "              of at most 7 significant and 10 fraction digits, exactly as the host parser reads them.  A chunk with\n"
    "              any other line (an exponent, nan, a tab, a malformed token ..) is parsed by the host, whole, so no\n"
    "              result changes and a malformed line ends the run as it does without the flag.  Prints per pass\n"
    "              `device parse: C chunks, B bytes, H parsed by the host (first at byte N)`.  Training, evaluation and\n"
    "              --predict_data read through the host parser unless --device_rows true is given as well.  Needs one of\n"
    "              the three passes; not with --cmd true.  (Environment FFM_TEXT_SLOT_BYTES sets the chunk size: a test\n"
    "              hook, results do not depend on it)\tdefault:false\n"
    "--device_rows <bool>: online training, evaluation and --predict_data read their files as raw bytes; the device parses\n"
    "              them (the grammar of --device_parse, a chunk with any other line parsed by the host, whole) and cuts the\n"
    "              parsed rows, in HBM, into the blocks the host would have cut, which the engine stages from there: no\n"
    "              entry is touched by the host or crosses PCIe a second time.  Losses, AUC / GAUC lines, scores, model\n"
    "              files and checkpoints do not change by a bit.  Prints per pass `device rows: <train|eval|predict> C\n"
    "              chunks, B bytes, H parsed by the host (first at byte N), K blocks`.  LR, FM and FFM; one GPU.  Not with\n"
    "              --online false, --cmd true, --n_gpus > 1, --compact_rows true, or sample weights (--pos_weight,\n"
    "              --neg_weight, --weight_data) on a run that trains; needs a file to read: --train_data with --n_epochs >\n"
    "              0, --eval_data or --predict_data.  --field_importance keeps reading --eval_data through the host\n"
    "              parser.  Independent of --device_parse (the counting passes); with both no text is parsed on the host\n"
    "              \tdefault:false\n";

static bool assign_bool(std::string arg) {
  std::transform(arg.begin(), arg.end(), arg.begin(), [](unsigned char c) { return std::tolower(c); });
  return arg == "true" || arg == "1";
}

std::string detect_file_type(const std::string &file_path) {
  std::ifstream ifs(file_path);
  if (!ifs.good()) {
    std::fprintf(stderr, "fail to open %s\n", file_path.c_str());
    std::exit(EXIT_FAILURE);
  }
  std::string line;
  std::getline(ifs, line);
  std::istringstream is(line);
  std::string label, first;
  is >> label >> first;
  const auto colons = std::count(first.begin(), first.end(), ':');
  if (colons == 1) return "libsvm";
  if (colons == 2) return "libffm";
  std::fprintf(stderr, "unknown file format...\n");
  std::exit(EXIT_FAILURE);
}

// The format a serving delta file names in its header (serve_delta.h: 8 bytes of magic, the version, then 32-bit
// little-endian fields, the format the sixth of them): "f32", "f16", or "" for anything else.  Read here by hand so
// that parsing options needs nothing but this file; the loader checks the whole header again.
static std::string serve_delta_format(const std::string &path) {
  unsigned char raw[36];
  std::FILE *f = std::fopen(path.c_str(), "rb");
  if (!f) return "";
  const size_t got = std::fread(raw, 1, sizeof raw, f);
  std::fclose(f);
  if (got != sizeof raw || std::string(reinterpret_cast<const char *>(raw), 8) != "FFMSDLT\n") return "";
  const unsigned format = raw[32] | raw[33] << 8 | raw[34] << 16 | static_cast<unsigned>(raw[35]) << 24;
  return format == 1 ? "f32" : format == 2 ? "f16" : "";
}

void config_options::parse_option(int argc, char *argv[]) {
  std::vector<std::string> args(argv + 1, argv + argc);
  if (args.size() % 2 != 0) throw std::invalid_argument("every option takes exactly one value");
  for (size_t i = 0; i < args.size(); i += 2) {
    const std::string &k = args[i], &v = args[i + 1];
    if (k == "--model_path") model_path = v;
    else if (k == "--model_type") {
      model_type = v;
      std::transform(model_type.begin(), model_type.end(), model_type.begin(),
                     [](unsigned char c) { return std::toupper(c); });
    }
    else if (k == "--online") online = assign_bool(v);
    else if (k == "--n_fields") n_fields = std::stoi(v);
    else if (k == "--n_feats") n_feats = std::stoi(v);
    else if (k == "--n_factors") n_factors = std::stoi(v);
    else if (k == "--train_data") train_path = v;
    else if (k == "--eval_data") eval_path = v;
    else if (k == "--init_mean") init_mean = std::stof(v);
    else if (k == "--init_stddev") init_stddev = std::stof(v);
    else if (k == "--w_alpha") w_alpha = std::stof(v);
    else if (k == "--w_beta") w_beta = std::stof(v);
    else if (k == "--w_l1") w_l1 = std::stof(v);
    else if (k == "--w_l2") w_l2 = std::stof(v);
    else if (k == "--n_threads") thread_num = std::stoi(v);
    else if (k == "--n_epochs") epoch = std::stoi(v);
    else if (k == "--checkpoint_path") checkpoint_path = v;
    else if (k == "--resume_from") resume_from = v;
    else if (k == "--cmd") cmd = assign_bool(v);
    else if (k == "--batch_size") batch_size = std::stoi(v);
    else if (k == "--batch_ramp") batch_ramp = std::stoi(v);
    else if (k == "--seed") seed = std::stoull(v);
    else if (k == "--device") device = std::stoi(v);
    else if (k == "--learn") learn = assign_bool(v);
    else if (k == "--refresh_weights") refresh_weights = assign_bool(v);
    else if (k == "--hash_feats") hash_feats = assign_bool(v);
    else if (k == "--normalize_rows") normalize_rows = assign_bool(v);
    else if (k == "--device_parse") device_parse = assign_bool(v);
    else if (k == "--device_rows") device_rows = assign_bool(v);
    else if (k == "--compact_rows") compact_rows = assign_bool(v);
    else if (k == "--field_importance") field_importance = assign_bool(v);
    else if (k == "--pair_importance") pair_importance = assign_bool(v);
    else if (k == "--pair_keep") {
      long long x = -1;
      size_t used = 0;
      try { x = std::stoll(v, &used); } catch (const std::exception &) { used = 0; }
      if (used != v.size() || used == 0 || x < 0 || x > 2080)
        throw std::invalid_argument("--pair_keep takes a number of pairs in [0, 2080], got `" + v + "`");
      pair_keep = static_cast<int>(x);
    }
    else if (k == "--pair_mask_out") pair_mask_out = v;
    else if (k == "--pair_curve") {
      // the form only: what the N may be depends on --n_fields, which may come later (checked below)
      pair_curve = v;
      pair_curve_keep.clear();
      if (v != "auto") {
        const std::string bad = "--pair_curve takes auto or 1 to 64 comma-separated numbers of pairs, got `" + v + "`";
        size_t at = 0;
        for (;;) {
          const size_t end = std::min(v.find(',', at), v.size());
          const std::string t = v.substr(at, end - at);
          if (t.empty() || t.size() > 4 || t.find_first_not_of("0123456789") != std::string::npos) throw std::invalid_argument(bad);
          if (pair_curve_keep.size() == 64) throw std::invalid_argument("--pair_curve takes at most 64 numbers of pairs (one pass has 64 cuts), got more");
          pair_curve_keep.push_back(std::stoi(t));
          if (end == v.size()) break;
          at = end + 1;
        }
      }
    }
    else if (k == "--pair_loss_budget") {
      double x = 0.0;
      size_t used = 0;
      try { x = std::stod(v, &used); } catch (const std::exception &) { used = 0; }
      if (used != v.size() || used == 0 || !std::isfinite(x))
        throw std::invalid_argument("--pair_loss_budget takes a finite per-row loss delta, got `" + v + "`");
      pair_loss_budget = x;
      pair_loss_budget_set = true;
    }
    else if (k == "--pair_mask") pair_mask = v;
    else if (k == "--n_gpus") n_gpus = std::stoi(v);
    else if (k == "--field_ranges") field_ranges = v;
    else if (k == "--field_ranges_out") field_ranges_out = v;
    else if (k == "--metrics") {
      if (v != "auc" && v != "none") throw std::invalid_argument("--metrics takes auc or none");
      metrics = v;
    }
    else if (k == "--pos_weight" || k == "--neg_weight") {
      float w = -1.0f;
      size_t used = 0;
      try { w = std::stof(v, &used); } catch (const std::exception &) { used = 0; }
      if (used != v.size() || used == 0 || !(w >= 0.0f) || w > 3.4028234e38f)
        throw std::invalid_argument(k + " takes a finite value >= 0, got `" + v + "`");
      (k == "--pos_weight" ? pos_weight : neg_weight) = w;
      weights_given = true;
    }
    else if (k == "--weight_data") { weight_path = v; weights_given = true; }
    else if (k == "--serve_weights") {
      if (v != "none" && v != "f32" && v != "f16") throw std::invalid_argument("--serve_weights takes none, f32 or f16");
      serve_weights = v;
    }
    else if (k == "--auc_key_field" || k == "--auc_key_rows") {
      long long x = 0;
      size_t used = 0;
      try { x = std::stoll(v, &used); } catch (const std::exception &) { used = 0; }
      if (used != v.size() || used == 0) throw std::invalid_argument(k + " takes an integer, got `" + v + "`");
      if (k == "--auc_key_rows") { auc_key_rows = x; continue; }
      if (x < 0 || x > 2147483647) throw std::invalid_argument("--auc_key_field names a field: >= 0, got `" + v + "`");
      auc_key_field = static_cast<int>(x);
    }
    else if (k == "--publish_path") {
      if (v.empty()) throw std::invalid_argument("--publish_path needs a file name prefix");
      publish_path = v;
    }
    else if (k == "--publish_weights") {
      if (v != "f32" && v != "f16") throw std::invalid_argument("--publish_weights takes f32 or f16");
      publish_weights = v;
    }
    else if (k == "--apply_deltas") {
      // PREFIX, or PREFIX:N with N a positive count (a prefix may hold colons itself: only a numeric tail counts)
      apply_deltas = v;
      apply_deltas_n = 0;
      const size_t colon = v.rfind(':');
      if (colon != std::string::npos && colon + 1 < v.size() &&
          std::all_of(v.begin() + static_cast<std::ptrdiff_t>(colon) + 1, v.end(), [](unsigned char c) { return std::isdigit(c); })) {
        long long n = 0;
        try { n = std::stoll(v.substr(colon + 1)); } catch (const std::exception &) { n = 0; }
        if (n <= 0 || n > 1000000) throw std::invalid_argument("--apply_deltas PREFIX:N takes a positive count, got `" + v + "`");
        apply_deltas = v.substr(0, colon);
        apply_deltas_n = static_cast<int>(n);
      }
      if (apply_deltas.empty()) throw std::invalid_argument("--apply_deltas needs a file name prefix");
    }
    else if (k == "--min_count" || k == "--rare_bits") {
      long long x = 0;
      size_t used = 0;
      try { x = std::stoll(v, &used); } catch (const std::exception &) { used = 0; }
      if (used != v.size() || used == 0) throw std::invalid_argument(k + " takes an integer, got `" + v + "`");
      if (k == "--min_count") {
        if (x < 0 || x > 65535) throw std::invalid_argument("--min_count takes a count in [0, 65535], got `" + v + "`");
        min_count = static_cast<int>(x);
      } else {
        if (x < 8 || x > 30) throw std::invalid_argument("--rare_bits takes a number of bits in [8, 30], got `" + v + "`");
        rare_bits = static_cast<int>(x);
      }
    }
    else if (k == "--n_buckets") {
      long long x = 0;
      size_t used = 0;
      try { x = std::stoll(v, &used); } catch (const std::exception &) { used = 0; }
      if (used != v.size() || used == 0 || x < 2 || x > 256)
        throw std::invalid_argument("--n_buckets takes a number of buckets in [2, 256], got `" + v + "`");
      n_buckets = static_cast<int>(x);
    }
    else if (k == "--bucket_fields") bucket_fields = v;
    else if (k == "--buckets") buckets = v;
    else if (k == "--buckets_out") buckets_out = v;
    else if (k == "--rare_ids") rare_ids = v;
    else if (k == "--rare_ids_out") rare_ids_out = v;
    else if (k == "--predict_data") predict_path = v;
    else if (k == "--predict_out") predict_out = v;
    else if (k == "--predict_output") {
      if (v != "prob" && v != "logit") throw std::invalid_argument("--predict_output takes prob or logit");
      predict_prob = v == "prob";
    }
    else throw std::invalid_argument("unknown argument: " + k + "\n");
  }
  if (predict_path.empty() != predict_out.empty())
    throw std::invalid_argument("--predict_data and --predict_out go together: one was given without the other");
  if (serve_weights != "none") {
    // a serving engine holds no accumulators: it can only score a saved model (refused here, before a device is opened)
    const std::string what = "--serve_weights " + serve_weights + " ";
    if (!publish_path.empty())
      throw std::invalid_argument("--publish_path publishes what training moved: a serving run (" + what + ") trains nothing");
    if (resume_from.empty() && apply_deltas.empty())
      throw std::invalid_argument(what + "scores a saved model: it needs --resume_from <checkpoint> --n_epochs 0");
    if (epoch > 0) throw std::invalid_argument(what + "cannot train: it needs --n_epochs 0 (got --n_epochs " + std::to_string(epoch) + ")");
    if (!model_path.empty()) throw std::invalid_argument(what + "writes no model: --model_path is not allowed with it");
    if (!checkpoint_path.empty()) throw std::invalid_argument(what + "holds no accumulators to checkpoint: --checkpoint_path is not allowed with it");
    if (n_gpus > 1) throw std::invalid_argument(what + "is one whole model on one GPU: --n_gpus > 1 is not allowed with it");
    if (refresh_weights)
      throw std::invalid_argument(what + "holds no accumulators to refresh from: write the checkpoint with --refresh_weights true instead");
    if (model_type != "FFM") throw std::invalid_argument(what + "is for FFM models only (got --model_type " + model_type + ")");
  }
  if (!publish_path.empty()) {
    // a shadow serving engine beside one whole FFM training engine (refused here, before a device is opened)
    const std::string what = "--publish_path " + publish_path + " ";
    if (model_type != "FFM") throw std::invalid_argument(what + "publishes a serving engine's rows: FFM only (got --model_type " + model_type + ")");
    if (n_gpus > 1) throw std::invalid_argument(what + "follows one whole model on one GPU: --n_gpus > 1 is not allowed with it");
    if (n_factors != 4 && n_factors != 8 && n_factors != 16 && n_factors != 32 && n_factors != 64)
      throw std::invalid_argument(what + "keeps a serving engine: --n_factors must be 4, 8, 16, 32 or 64 (got " + std::to_string(n_factors) + ")");
    if (cmd) throw std::invalid_argument(what + "publishes after an epoch over --train_data: --cmd true has none");
  }
  if (!apply_deltas.empty()) {
    // a fresh serving engine plus the published deltas (refused here, before a device is opened)
    const std::string what = "--apply_deltas " + apply_deltas + " ";
    if (serve_weights == "none") throw std::invalid_argument(what + "fills a serving engine: it needs --serve_weights f32 or f16");
    if (!resume_from.empty()) throw std::invalid_argument(what + "starts from a fresh serving engine: --resume_from is not allowed with it");
    if (epoch > 0) throw std::invalid_argument(what + "cannot train: it needs --n_epochs 0 (got --n_epochs " + std::to_string(epoch) + ")");
    const std::string first = apply_deltas + ".1.delta";
    const std::string fmt = serve_delta_format(first);
    if (fmt.empty()) throw std::invalid_argument(what + "needs at least " + first + ": no serving delta of that name can be read");
    if (fmt != serve_weights)
      throw std::invalid_argument(what + "holds " + fmt + " rows (" + first + "): --serve_weights " + serve_weights + " cannot take them");
  }
  if (field_ranges == "counted") {
    // the counting pass reads the training file on one GPU before an FFM model exists (refused here, before a device is opened)
    const std::string what = "--field_ranges counted ";
    if (model_type != "FFM") throw std::invalid_argument(what + "counts the ids of fields, which only FFM rows have (got --model_type " + model_type + ")");
    if (!resume_from.empty())
      throw std::invalid_argument(what + "is not allowed with --resume_from: a saved model's ranges are the ones it was trained with; "
                                         "write them with --field_ranges_out and pass --field_ranges @FILE");
    if (train_path.empty()) throw std::invalid_argument(what + "counts the ids of the training file: it needs --train_data");
    if (n_gpus > 1) throw std::invalid_argument(what + "sizes the ranges of one whole model on one GPU: --n_gpus > 1 is not allowed with it");
  }
  if (!field_ranges.empty() && field_ranges[0] == '@') {
    if (field_ranges.size() == 1) throw std::invalid_argument("--field_ranges @FILE needs a file name after the @");
    if (model_type != "FFM")
      throw std::invalid_argument("--field_ranges " + field_ranges + " names the ranges of fields, which only FFM has (got --model_type " + model_type + ")");
  }
  if (!field_ranges_out.empty()) {
    const bool ranged = field_ranges == "uniform" || field_ranges == "counted" || field_ranges[0] == '@';
    if (!ranged || model_type != "FFM")
      throw std::invalid_argument("--field_ranges_out writes the fields' id ranges: it needs an FFM model and --field_ranges uniform, counted or @FILE");
  }
  if (device_parse) {
    // only the counting pre-passes read text through the device parser (refused here, before a device is opened)
    if (min_count <= 1 && bucket_fields.empty() && field_ranges != "counted")
      throw std::invalid_argument("--device_parse true parses the text of the counting passes on the device: it needs --min_count > 1, "
                                  "--bucket_fields or --field_ranges counted (training and evaluation read through the device with --device_rows true)");
    if (cmd) throw std::invalid_argument("--device_parse true is not allowed with --cmd true");
  }
  if (device_rows) {
    // the rows of one engine's online passes are cut in HBM (refused here, before a device is opened)
    const std::string what = "--device_rows true ";
    if (!online)
      throw std::invalid_argument(what + "cuts the blocks of a file read in order: --online false loads whole files and shuffles them on the host");
    if (cmd) throw std::invalid_argument(what + "reads files: --cmd true is not allowed with it");
    if (n_gpus > 1) throw std::invalid_argument(what + "feeds one whole model on one GPU: --n_gpus > 1 is not allowed with it");
    if (compact_rows)
      throw std::invalid_argument(what + "is not allowed with --compact_rows true: the arrays never cross PCIe on this path");
    if (weights_given && epoch > 0)
      throw std::invalid_argument(what + "trains without sample weights, which are filled from labels on the host: --pos_weight / "
                                         "--neg_weight / --weight_data are not allowed with it while --n_epochs > 0");
    if (!(epoch > 0 && !train_path.empty()) && eval_path.empty() && predict_path.empty())
      throw std::invalid_argument(what + "needs a file to read: --train_data with --n_epochs > 0, --eval_data or --predict_data");
  }
  // a row's length is a sum over all of its entries (refused here, before a device is opened)
  if (normalize_rows && n_gpus > 1)
    throw std::invalid_argument("--normalize_rows true scales whole rows, which a shard does not own: --n_gpus > 1 is not allowed with it");
  if (min_count > 1 || !rare_ids.empty()) {
    // the fold works on raw ids, on one whole model on one GPU (refused here, before a device is opened)
    const std::string what = min_count > 1 ? "--min_count " + std::to_string(min_count) + " " : "--rare_ids " + rare_ids + " ";
    if (min_count > 1 && !rare_ids.empty())
      throw std::invalid_argument("--min_count counts a keep-map and --rare_ids names one: give one of the two");
    if (!rare_ids.empty() && (rare_ids[0] != '@' || rare_ids.size() == 1))
      throw std::invalid_argument("--rare_ids takes @FILE, the keep-map --rare_ids_out wrote, got `" + rare_ids + "`");
    if (!hash_feats) throw std::invalid_argument(what + "folds raw ids before they are hashed: it needs --hash_feats true");
    if (n_gpus > 1) throw std::invalid_argument(what + "folds on one whole model on one GPU: --n_gpus > 1 is not allowed with it");
    if (min_count > 1 && !resume_from.empty())
      throw std::invalid_argument(what + "is not allowed with --resume_from: a saved model's keep-map is the one it was trained with; "
                                         "write it with --rare_ids_out and pass --rare_ids @FILE");
    if (min_count > 1 && train_path.empty()) throw std::invalid_argument(what + "counts the ids of the training file: it needs --train_data");
  }
  if (!rare_ids_out.empty() && min_count <= 1 && rare_ids.empty())
    throw std::invalid_argument("--rare_ids_out writes the keep-map of rare ids: it needs --min_count > 1 or --rare_ids @FILE");
  if (!bucket_fields.empty() || !buckets.empty()) {
    // buckets become raw ids of one whole FFM model on one GPU (refused here, before a device is opened)
    const std::string what = !bucket_fields.empty() ? "--bucket_fields " + bucket_fields + " " : "--buckets " + buckets + " ";
    if (!bucket_fields.empty() && !buckets.empty())
      throw std::invalid_argument("--bucket_fields counts a bucket table and --buckets names one: give one of the two");
    if (!buckets.empty() && (buckets[0] != '@' || buckets.size() == 1))
      throw std::invalid_argument("--buckets takes @FILE, the table --buckets_out wrote, got `" + buckets + "`");
    if (!hash_feats) throw std::invalid_argument(what + "turns values into ids that are then hashed: it needs --hash_feats true");
    if (model_type != "FFM") throw std::invalid_argument(what + "buckets the values of fields, which only FFM rows have (got --model_type " + model_type + ")");
    if (n_gpus > 1) throw std::invalid_argument(what + "buckets on one whole model on one GPU: --n_gpus > 1 is not allowed with it");
    if (!bucket_fields.empty()) {
      if (!resume_from.empty())
        throw std::invalid_argument(what + "is not allowed with --resume_from: a saved model's buckets are the ones it was trained with; "
                                           "write them with --buckets_out and pass --buckets @FILE");
      if (train_path.empty()) throw std::invalid_argument(what + "counts the values of the training file: it needs --train_data");
      // LIST: items a or a-b, comma separated
      std::vector<char> chosen(static_cast<size_t>(std::max(n_fields, 0)), 0);
      size_t at = 0;
      const std::string &s = bucket_fields;
      auto number = [&]() -> long long {
        const size_t from = at;
        while (at < s.size() && std::isdigit(static_cast<unsigned char>(s[at]))) at++;
        if (at == from || at - from > 9) throw std::invalid_argument("--bucket_fields takes a list such as 0-12,20, got `" + s + "`");
        return std::stoll(s.substr(from, at - from));
      };
      for (;;) {
        const long long a = number();
        long long b = a;
        if (at < s.size() && s[at] == '-') {
          at++;
          b = number();
        }
        if (b < a) throw std::invalid_argument("--bucket_fields takes a list such as 0-12,20, got `" + s + "`");
        if (b >= n_fields)
          throw std::invalid_argument(what + "names field " + std::to_string(b) + ", which is not a field of this model: --n_fields is " + std::to_string(n_fields));
        for (long long f = a; f <= b; f++) chosen[static_cast<size_t>(f)] = 1;
        if (at == s.size()) break;
        if (s[at] != ',') throw std::invalid_argument("--bucket_fields takes a list such as 0-12,20, got `" + s + "`");
        at++;
      }
      bucket_field_list.clear();
      for (int f = 0; f < n_fields; f++)
        if (chosen[static_cast<size_t>(f)]) bucket_field_list.push_back(f);
    }
  }
  if (!buckets_out.empty() && bucket_fields.empty() && buckets.empty())
    throw std::invalid_argument("--buckets_out writes the bucket table: it needs --bucket_fields or --buckets @FILE");
  if (auc_key_field >= 0) {
    // the grouped AUC rides on the AUC lines of one whole FFM model (refused here, before a device is opened)
    const std::string what = "--auc_key_field " + std::to_string(auc_key_field) + " ";
    if (metrics != "auc") throw std::invalid_argument(what + "adds a line to the AUC lines: it needs --metrics auc");
    if (model_type != "FFM") throw std::invalid_argument(what + "names a field, which only FFM rows have (got --model_type " + model_type + ")");
    if (n_gpus > 1) throw std::invalid_argument(what + "is kept by one whole model on one GPU: --n_gpus > 1 is not allowed with it");
    if (auc_key_field >= n_fields)
      throw std::invalid_argument(what + "is not a field of this model: --n_fields is " + std::to_string(n_fields));
    if (auc_key_rows <= 0) throw std::invalid_argument("--auc_key_rows must be positive, got " + std::to_string(auc_key_rows));
  }
  // --field_importance, --pair_importance: one more pass over the eval file through one whole FFM model's wave kernel,
  // with a variant per `things` (refused here, before a device is opened)
  auto check_importance = [&](const std::string &what, const std::string &things, const std::string &keeps) {
    if (eval_path.empty()) throw std::invalid_argument(what + "ablates the " + things + " on the evaluation file: it needs --eval_data");
    if (model_type != "FFM") throw std::invalid_argument(what + "drops " + things + ", which only FFM rows have (got --model_type " + model_type + ")");
    if (n_gpus > 1) throw std::invalid_argument(what + "runs on one whole model on one GPU: --n_gpus > 1 is not allowed with it");
    if (n_fields > 64) throw std::invalid_argument(what + keeps + ": --n_fields is " + std::to_string(n_fields) + ", at most 64");
    if (n_factors != 4 && n_factors != 8 && n_factors != 16 && n_factors != 32 && n_factors != 64)
      throw std::invalid_argument(what + "runs the one-wave-per-row kernel: --n_factors must be 4, 8, 16, 32 or 64 (got " +
                                  std::to_string(n_factors) + ")");
  };
  if (field_importance) check_importance("--field_importance true ", "fields", "keeps one lane of a 64-lane wave per field");
  if (pair_importance)
    check_importance("--pair_importance true ", "field pairs", "keeps the pairs of at most 64 fields in the registers of a 64-lane wave");
  // --pair_curve LIST|auto, --pair_loss_budget T: the pruning curve behind the pair importance pass, and the mask its
  // budget picks (refused here, before a device is opened)
  if (!pair_curve.empty()) {
    if (!pair_importance)
      throw std::invalid_argument("--pair_curve " + pair_curve + " ranks the pairs by the pair importance pass: it needs --pair_importance true");
    const int V = n_fields * (n_fields + 1) / 2;
    if (pair_curve == "auto") {
      pair_curve_keep.clear();
      for (int i = 0; i < 64; i++) pair_curve_keep.push_back((2 * i * V + 63) / 126);  // round(i V / 63): never a tie
    }
    for (int n : pair_curve_keep)
      if (n > V)
        throw std::invalid_argument("--pair_curve " + pair_curve + ": " + std::to_string(n) + " is more than the " + std::to_string(V) +
                                    " pairs of --n_fields " + std::to_string(n_fields));
    std::sort(pair_curve_keep.begin(), pair_curve_keep.end());
    pair_curve_keep.erase(std::unique(pair_curve_keep.begin(), pair_curve_keep.end()), pair_curve_keep.end());
  }
  if (pair_loss_budget_set) {
    if (pair_keep >= 0)
      throw std::invalid_argument("--pair_loss_budget picks the number of pairs --pair_keep would give: the two are not allowed together");
    if (pair_curve.empty()) throw std::invalid_argument("--pair_loss_budget picks from the curve's listed numbers of pairs: it needs --pair_curve");
    if (pair_mask_out.empty()) throw std::invalid_argument("--pair_loss_budget picks the pairs --pair_mask_out FILE writes: it needs --pair_mask_out");
  }
  // --pair_keep N --pair_mask_out FILE: the pair importance pass's answer as a mask file (refused here, before a device is opened)
  if (pair_keep >= 0 || (!pair_mask_out.empty() && !pair_loss_budget_set)) {
    if (pair_keep < 0) throw std::invalid_argument("--pair_mask_out writes the pairs --pair_keep N selects: it needs --pair_keep");
    if (pair_mask_out.empty()) throw std::invalid_argument("--pair_keep selects the pairs --pair_mask_out FILE writes: it needs --pair_mask_out");
    if (!pair_importance)
      throw std::invalid_argument("--pair_keep " + std::to_string(pair_keep) + " ranks the pairs by the pair importance pass: it needs --pair_importance true");
    const int V = n_fields * (n_fields + 1) / 2;
    if (pair_keep > V)
      throw std::invalid_argument("--pair_keep " + std::to_string(pair_keep) + " is more than the " + std::to_string(V) + " pairs of --n_fields " + std::to_string(n_fields));
  }
  // --pair_mask @FILE: one whole FFM model that trains nothing predicts with the kept pairs (refused here, before a device is opened)
  if (!pair_mask.empty()) {
    const std::string what = "--pair_mask " + pair_mask + " ";
    if (pair_mask[0] != '@' || pair_mask.size() == 1)
      throw std::invalid_argument("--pair_mask takes @FILE, the mask --pair_mask_out wrote, got `" + pair_mask + "`");
    if (epoch > 0) throw std::invalid_argument(what + "masks prediction, not training: it needs --n_epochs 0 (got --n_epochs " + std::to_string(epoch) + ")");
    if (field_importance) throw std::invalid_argument(what + "is not allowed with --field_importance true: the variants are the whole model's");
    if (pair_importance) throw std::invalid_argument(what + "is not allowed with --pair_importance true: the variants are the whole model's");
    if (n_gpus > 1) throw std::invalid_argument(what + "masks one whole model on one GPU: --n_gpus > 1 is not allowed with it");
    if (model_type != "FFM") throw std::invalid_argument(what + "names field pairs, which only FFM rows have (got --model_type " + model_type + ")");
    if (cmd) throw std::invalid_argument(what + "scores files: --cmd true is not allowed with it");
    if (n_fields > 64) throw std::invalid_argument(what + "keeps a field's partners in one 64-bit word: --n_fields is " + std::to_string(n_fields) + ", at most 64");
    if (n_factors != 4 && n_factors != 8 && n_factors != 16 && n_factors != 32 && n_factors != 64)
      throw std::invalid_argument(what + "runs the one-wave-per-row kernel: --n_factors must be 4, 8, 16, 32 or 64 (got " + std::to_string(n_factors) + ")");
  }
  // (--n_epochs 0 with a file to score needs no training file: the format is then the scored file's)
  file_type = detect_file_type(train_path.empty() && epoch == 0 && !predict_path.empty() ? predict_path : train_path);
  if (model_type == "FFM" && file_type != "libffm") {
    std::fprintf(stderr, "FFM model requires libffm data format...\n");
    std::exit(EXIT_FAILURE);
  }
}
