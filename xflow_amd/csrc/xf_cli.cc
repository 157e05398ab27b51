// xf_cli.cc — `xflow_lr <train_prefix> <test_prefix> <model 0|1> <epochs> [name=value ...]`
// Same positional arguments as the reference's entry point (src/model/main.cc:27-44).  Started
// by the reference's scripts/local.sh it behaves like this: DMLC_ROLE=scheduler and =server
// have nothing to do (the "servers" are the key-range shards of the table in the workers' HBM,
// rank 0 is the rendezvous) and return at once; every DMLC_ROLE=worker is one GPU of a run of
// DMLC_NUM_WORKER, meeting the others at DMLC_PS_ROOT_URI:DMLC_PS_ROOT_PORT.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <string>

#include "xf_worker.h"

int main(int argc, char *argv[]) {
  if (argc < 5) {
    std::cout << "usage: xflow_lr <train_prefix> <test_prefix> <model: 0 LR | 1 FM> <epochs>"
                 " [name=value ...]\n"
              << "LR model example: xflow_lr data/small_train data/small_test 0 100\n"
              << "FM model example: xflow_lr data/small_train data/small_test 1 100\n"
              << "Rendle's FM (per-factor second-order term, one worker): append fm_mode=canonical\n"
              << "field-aware FM (k factors per field, one worker; fgid in [0, N)): append "
                 "fm_mode=field_aware fields=N\n"
              << "feature values (x = val of fgid:fid:val instead of 1; LR, or FM with "
                 "fm_mode=canonical or field_aware; one worker): append feature_values=on\n"
              << "text tokenised on the GPU: append ingest=gpu (keys only) or ingest=gpu_fields "
                 "(also fgid and val, for field_aware and feature_values)\n"
              << "feature admission (a key enters the model once a counting Bloom filter has seen "
                 "it N times; one worker): append admit_count=N [admit_log2_slots=26 "
                 "admit_hashes=3]; several workers sharing one filter: admit_shared=1\n"
              << "negative subsampling (every positive row kept, a negative with probability r, "
                 "a kept negative's loss weighted by 1 / r): append neg_keep=r\n"
              << "feature crosses (a nonzero per listed pair of fields and per pair of their "
                 "members, formed on the GPU; predict needs the same spec): append cross=2*3,16*17 "
                 "[cross_fgid_base=N with fm_mode=field_aware]\n"
              << "row normalisation (every row scaled to unit L2 length on the GPU, behind the "
                 "crosses and admission; needs feature_values=on; predict needs the same "
                 "setting): append row_norm=l2\n"
              << "held-out validation (a hash-chosen share r of the training rows is never trained "
                 "on and scored after every E-th epoch; stop after P validated epochs without "
                 "improvement): append holdout=r [holdout_every=E early_stop=P "
                 "early_stop_delta=d]\n"
              << "progressive validation (per epoch: logloss and AUC of every training row under "
                 "the weights it met before it was trained on, counted on the GPU): append "
                 "progress=1\n"
              << "... and per value of one field (which site, advertiser or slot is miscalibrated "
                 "or carries the loss): append progress_by=F [progress_slots=16 progress_top=10 "
                 "progress_slices_out=PATH]\n";
    return 2;
  }
  if (const char *role = getenv("DMLC_ROLE")) {  // main.cc:22-26: ps::IsServer / scheduler
    if (!strcmp(role, "scheduler") || !strcmp(role, "server")) {
      std::cout << "xflow_lr: no " << role << " process in this build (the table lives in the "
                << "workers' HBM)" << std::endl;
      return 0;
    }
  }
  const int model = argv[3][0] - '0';
  if (model == 2) {
    std::cerr << "MVM (model 2) is out of scope of this build (SURVEY.md §2 row 11)\n";
    return 2;
  }
  xflow_amd::Worker *worker;
  if (model == 0) {
    std::cout << "start LR " << std::endl;
    worker = new xflow_amd::LRWorker(argv[1], argv[2]);
  } else {
    std::cout << "start FM " << std::endl;
    worker = new xflow_amd::FMWorker(argv[1], argv[2]);
  }
  worker->epochs = std::atoi(argv[4]);
  for (int i = 5; i < argc; ++i) {
    std::string kv = argv[i];
    const size_t eq = kv.find('=');
    if (eq == std::string::npos ||
        worker->set_param(kv.substr(0, eq).c_str(), kv.substr(eq + 1).c_str()) != XF_OK) {
      std::cerr << "bad option '" << kv << "': " << xf_last_error() << "\n";
      return 2;
    }
  }
  const int rc = worker->train();
  if (rc != XF_OK) {
    std::cerr << "xflow_lr: error " << rc << ": " << xf_last_error() << "\n";
    return 1;
  }
  if (worker->admit_count && worker->admit_shared) {  // (the filter's stats stay per rank)
    double seen = 0, kept = 0;
    worker->get_metric("admit_seen", &seen);
    worker->get_metric("admit_kept", &kept);
    std::cout << "rank " << worker->rank << " admit_seen = " << (unsigned long long)seen
              << " admit_kept = " << (unsigned long long)kept << std::endl;
  }
  if (worker->neg_keep < 1.0f) {  // (every rank samples its own rows)
    double seen = 0, kept = 0, rows = 0;
    worker->get_metric("neg_seen", &seen);
    worker->get_metric("neg_kept", &kept);
    worker->get_metric("rows_kept", &rows);
    std::cout << "rank " << worker->rank << " neg_seen = " << (unsigned long long)seen
              << " neg_kept = " << (unsigned long long)kept << " rows_kept = "
              << (unsigned long long)rows << std::endl;
  }
  if (!worker->cross_spec.empty()) {  // (every rank crosses its own rows)
    double in = 0, out = 0;
    worker->get_metric("cross_in", &in);
    worker->get_metric("cross_out", &out);
    std::cout << "rank " << worker->rank << " cross_in = " << (unsigned long long)in
              << " cross_out = " << (unsigned long long)out << std::endl;
  }
  double eps = 0;
  worker->get_metric("examples_per_sec", &eps);
  std::cout << "examples/sec (train loop): " << eps << std::endl;
  delete worker;
  return 0;
}
