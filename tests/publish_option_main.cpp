// Stand-alone check of host/cmd_option.cpp's --publish_path / --publish_weights / --apply_deltas: the defaults, the
// accepted forms, and every refusal, all out of parse_option (no device, no engine).  argv[1]: a libffm file,
// argv[2]: a scratch directory.  Built and run by tests/test_publish_host.py.
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../ftrl-ffm_amd/host/cmd_option.h"
#include "../include/ffm_engine.h"

static int g_failed = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failed++; } \
  } while (0)

static config_options parse(std::vector<std::string> args) {
  std::vector<char *> argv{const_cast<char *>("prog")};
  for (auto &a : args) argv.push_back(a.data());
  config_options opt;
  opt.parse_option(static_cast<int>(argv.size()), argv.data());
  return opt;
}
static void refused(const char *name, std::vector<std::string> args, const char *expect) {
  std::string msg;
  bool thrown = false;
  try {
    (void)parse(std::move(args));
  } catch (const std::invalid_argument &e) {
    thrown = true;
    msg = e.what();
  }
  if (!thrown || msg.find(expect) == std::string::npos) {
    std::printf("FAIL refuse %s: %s\n", name, thrown ? msg.c_str() : "accepted");
    g_failed++;
  } else {
    std::printf("refuse %-34s ok (%s)\n", name, msg.c_str());
  }
}
// the first 36 bytes of a serving delta: magic, version, five 32-bit fields, the format
static void fake_delta(const std::string &path, unsigned format) {
  std::string b("FFMSDLT\n", 8);
  const unsigned words[7] = {1, 2, 10000, 8, 16, 0, format};
  for (unsigned w : words)
    for (int i = 0; i < 4; i++) b.push_back(static_cast<char>((w >> (8 * i)) & 0xff));
  std::ofstream(path, std::ios::binary).write(b.data(), static_cast<std::streamsize>(b.size()));
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  const std::string data = argv[1], dir = argv[2];
  using V = std::vector<std::string>;
  CHECK(FFM_ENGINE_ABI_VERSION == 4);
  {
    const config_options d = parse({"--train_data", data});
    CHECK(d.publish_path.empty() && d.publish_weights == "f32" && d.apply_deltas.empty() && d.apply_deltas_n == 0);
    CHECK(d.serve_weights == "none" && d.model_type == "FFM" && d.n_gpus == 1 && !d.refresh_weights);
  }
  {
    const config_options o = parse({"--train_data", data, "--publish_path", dir + "/P"});
    CHECK(o.publish_path == dir + "/P" && o.publish_weights == "f32");
    const config_options h = parse({"--train_data", data, "--publish_path", "P", "--publish_weights", "f16", "--n_factors", "64"});
    CHECK(h.publish_weights == "f16" && h.n_factors == 64);
  }
  const V pub = {"--train_data", data, "--publish_path", "P"};
  auto with = [](V a, const V &b) { a.insert(a.end(), b.begin(), b.end()); return a; };
  refused("--publish_weights f8", with(pub, {"--publish_weights", "f8"}), "f32 or f16");
  refused("publish LR", {"--train_data", data, "--publish_path", "P", "--model_type", "LR"}, "FFM only");
  refused("publish FM", {"--train_data", data, "--publish_path", "P", "--model_type", "FM"}, "FFM only");
  refused("publish --n_gpus 2", with(pub, {"--n_gpus", "2"}), "--n_gpus");
  refused("publish --n_factors 12", with(pub, {"--n_factors", "12"}), "--n_factors");
  refused("publish --cmd true", with(pub, {"--cmd", "true"}), "--cmd");
  refused("publish --serve_weights f32", with(pub, {"--serve_weights", "f32", "--resume_from", "ck", "--n_epochs", "0"}), "trains nothing");

  fake_delta(dir + "/A.1.delta", 1);
  fake_delta(dir + "/H.1.delta", 2);
  const V score = {"--predict_data", data, "--predict_out", dir + "/out.txt", "--n_epochs", "0"};
  {
    const config_options o = parse(with(score, {"--serve_weights", "f32", "--apply_deltas", dir + "/A"}));
    CHECK(o.apply_deltas == dir + "/A" && o.apply_deltas_n == 0 && o.serve_weights == "f32");
    const config_options n = parse(with(score, {"--serve_weights", "f16", "--apply_deltas", dir + "/H:2"}));
    CHECK(n.apply_deltas == dir + "/H" && n.apply_deltas_n == 2);
  }
  refused("apply without --serve_weights", with(score, {"--apply_deltas", dir + "/A"}), "--serve_weights");
  refused("apply with --resume_from", with(score, {"--serve_weights", "f32", "--apply_deltas", dir + "/A", "--resume_from", "ck"}), "--resume_from");
  refused("apply with --n_epochs 1", {"--train_data", data, "--n_epochs", "1", "--serve_weights", "f32", "--apply_deltas", dir + "/A"}, "--n_epochs");
  refused("apply f32 files as f16", with(score, {"--serve_weights", "f16", "--apply_deltas", dir + "/A"}), "f32 rows");
  refused("apply f16 files as f32", with(score, {"--serve_weights", "f32", "--apply_deltas", dir + "/H"}), "f16 rows");
  refused("apply without a first file", with(score, {"--serve_weights", "f32", "--apply_deltas", dir + "/none"}), "none.1.delta");
  refused("apply PREFIX:0", with(score, {"--serve_weights", "f32", "--apply_deltas", dir + "/A:0"}), "positive count");
  std::printf("%d failed\n", g_failed);
  return g_failed ? 1 : 0;
}
