// Text in, text out, everything between on the device: read a Matrix Market file (MTXReader parses it on the GPU),
// reorder it with RCM, permute rows and columns, and write the permuted matrix as a Matrix Market file and, if asked,
// as an edge list (io/mtx_writer.h, io/edge_list_writer.h format on the GPU).  Values are written with 9 significant
// digits, so that the float values of the file read back bit-identical.
// Usage: text_tool [--symmetrize] <in.mtx> <out.mtx> [out.edges]
// Without --symmetrize the pattern must be structurally symmetric (RCM refuses any other).  With it the order comes from
// the pattern of A + A^T (reorder::RCMReorderParams::symmetrize); the matrix written is the permuted ORIGINAL.
#include <cstring>
#include <iostream>

#include "sparsebase/sparsebase.h"

using namespace sparsebase;

int main(int argc, char *argv[]) {
  const bool symmetrize = argc > 1 && std::strcmp(argv[1], "--symmetrize") == 0;
  if (symmetrize) {
    argc--;
    argv++;
  }
  if (argc < 3) {
    std::cout << "Usage: ./text_tool [--symmetrize] <matrix_market_format> <out.mtx> [out.edges]\n";
    return 1;
  }
  try {
    context::HIPContext gpu(hip::DefaultDevice());
    io::MTXReader<int, int, float> reader(argv[1]);
    std::unique_ptr<format::HIPCOO<int, int, float>> coo(reader.ReadHIPCOO(gpu));
    std::unique_ptr<format::HIPCSR<int, int, float>> csr(coo->Convert<format::HIPCSR>(&gpu));
    std::cout << "Number of vertices: " << csr->get_dimensions()[0] << "\nNumber of edges: " << csr->get_num_nnz() << std::endl;
    std::unique_ptr<format::HIPArray<int>> order(
        bases::ReorderBase::Reorder<reorder::RCMReorder>(reorder::RCMReorderParams(symmetrize), csr.get(), gpu));
    std::unique_ptr<format::HIPCSR<int, int, float>> permuted(
        bases::ReorderBase::Permute2D<format::HIPCSR>(order.get(), csr.get(), {&gpu}, true));
    io::MTXWriter<int, int, float>(argv[2], "matrix", "coordinate", "real", "general", 9).WriteHIPCSR(permuted.get());
    std::cout << "wrote " << argv[2] << std::endl;
    if (argc > 3) {
      io::EdgeListWriter<int, int, float>(argv[3], true, 9).WriteHIPCSR(permuted.get());
      std::cout << "wrote " << argv[3] << std::endl;
    }
  } catch (std::exception &e) {
    std::cerr << "text_tool: " << e.what() << std::endl;
    return 2;
  }
  return 0;
}
