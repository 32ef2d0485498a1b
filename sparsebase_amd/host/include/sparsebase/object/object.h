// sparsebase/object/object.h — Object, AbstractObject, Graph and HyperGraph (reference: object/object.h:28-87,
// object/object.cc:12-158): a connectivity Format held with or without ownership, and for a Graph its dimensions, the
// number of vertex weights and the per-vertex weight arrays, all public as in the reference.  The connectivity may be a
// host or a device format.
//
// HyperGraph is a Graph whose connectivity is the nets x cells CSR (n_ nets, m_ pins: the pins of a net in file order, in
// the file's base), with the cells x nets CSR beside it (xNetCSR_), the weights of the nets and of the cells, the base
// the ids are in and the number of constraints: the reference's two constructors and public members.  One member more:
// xNetHIPCSR_, the cells x nets side of a hypergraph that PatohReader::ReadHIPHyperGraph left on the device (xNetCSR_ is
// null there).  What a reader allocates — the cells x nets CSR and the two weight arrays — is owned by the HyperGraph it
// returns (OwnParts) and freed with it; a HyperGraph constructed from a caller's parts does not own them.
//
// One thing more than the reference: the weight arrays that MetisGraphReader::ReadGraph allocates are owned by the Graph
// it returns (OwnVertexWeights) and freed with it; the reference leaks them.  A Graph constructed from a caller's
// vertexWeights table does not own it, as in the reference.  Copies take the connectivity only (object.cc:69-82).
#ifndef SPARSEBASE_OBJECT_OBJECT_H_
#define SPARSEBASE_OBJECT_OBJECT_H_
#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "sparsebase/format/array.h"
#include "sparsebase/format/coo.h"
#include "sparsebase/format/csr.h"
#include "sparsebase/format/format.h"
#include "sparsebase/format/hip_formats.h"

namespace sparsebase::io {
template <typename I, typename N, typename V>
class MTXReader;
template <typename I, typename N, typename V>
class EdgeListReader;
}  // namespace sparsebase::io

namespace sparsebase::object {

class Object {
 public:
  virtual ~Object() = default;
  virtual void VerifyStructure() = 0;
};

template <typename IDType, typename NNZType, typename ValueType>
class AbstractObject : public Object {
 protected:
  std::unique_ptr<format::Format, std::function<void(format::Format *)>> connectivity_;

 public:
  ~AbstractObject() override = default;
  AbstractObject() : connectivity_(nullptr, format::BlankDeleter<format::Format>()) {}
  AbstractObject(const AbstractObject &rhs)
      : connectivity_(rhs.connectivity_ ? rhs.connectivity_->Clone() : nullptr, std::default_delete<format::Format>()) {}
  AbstractObject(AbstractObject &&rhs) : connectivity_(std::move(rhs.connectivity_)) {
    rhs.connectivity_ = {nullptr, format::BlankDeleter<format::Format>()};
  }
  format::Format *get_connectivity() const { return connectivity_.get(); }
  format::Format *release_connectivity() {
    format::Format *raw = connectivity_.release();
    connectivity_ = {raw, format::BlankDeleter<format::Format>()};
    return raw;
  }
  void set_connectivity(format::Format *conn, bool own) {
    if (own) connectivity_ = {conn, std::default_delete<format::Format>()};
    else connectivity_ = {conn, format::BlankDeleter<format::Format>()};
  }
  bool ConnectivityIsOwned() const {
    return connectivity_.get_deleter().target_type() != typeid(format::BlankDeleter<format::Format>);
  }
};

template <typename VertexID, typename NumEdges, typename Weight>
class Graph : public AbstractObject<VertexID, NumEdges, Weight> {
 public:
  explicit Graph(format::Format *connectivity) {
    this->set_connectivity(connectivity, true);
    this->VerifyStructure();
    InitializeInfoFromConnection();
  }
  Graph(format::Format *connectivity, NumEdges ncon, format::Array<Weight> **vertexWeights) : Graph(connectivity) {
    ncon_ = ncon;
    vertexWeights_ = vertexWeights;
  }
  Graph() = default;
  Graph(const Graph &rhs) : AbstractObject<VertexID, NumEdges, Weight>(rhs) { InitializeInfoFromConnection(); }
  Graph(Graph &&rhs) : AbstractObject<VertexID, NumEdges, Weight>(std::move(rhs)) {
    InitializeInfoFromConnection();
    ncon_ = rhs.ncon_;
    vertexWeights_ = rhs.vertexWeights_;
    release_weights_ = std::move(rhs.release_weights_);
    rhs.release_weights_ = nullptr;
    rhs.vertexWeights_ = nullptr;
  }
  Graph &operator=(const Graph &rhs) {
    if (this != &rhs) {
      this->set_connectivity(rhs.get_connectivity() ? rhs.get_connectivity()->Clone() : nullptr, true);
      InitializeInfoFromConnection();
    }
    return *this;
  }
  ~Graph() override {
    if (release_weights_) release_weights_();
  }
  template <typename Reader>
  void ReadConnectivityToCSR(const Reader &reader) {
    Adopt(reader.ReadCSR());
  }
  template <typename Reader>
  void ReadConnectivityToCOO(const Reader &reader) {
    Adopt(reader.ReadCOO());
  }
  // (io::MTXReader and io::EdgeListReader are only declared above: a caller of these two includes io/mtx_reader.h or
  // io/edge_list_reader.h, so that the reader is complete where the member is instantiated; sparsebase.h includes both)
  void ReadConnectivityFromMTXToCOO(std::string filename) { Adopt(io::MTXReader<VertexID, NumEdges, Weight>(filename).ReadCOO()); }
  void ReadConnectivityFromEdgelistToCSR(std::string filename) {
    Adopt(io::EdgeListReader<VertexID, NumEdges, Weight>(filename, false, false, false, true, true).ReadCSR());
  }
  void InitializeInfoFromConnection() {
    if (!this->get_connectivity()) return;
    n_ = (VertexID)this->get_connectivity()->get_dimensions()[0];
    m_ = (NumEdges)this->get_connectivity()->get_num_nnz();
  }
  void VerifyStructure() override {
    if (this->get_connectivity()->get_order() != 2) throw -1;  // (object.cc:156)
  }
  // the Graph frees `table` and the `count` arrays it points to when it dies (what a reader allocated for it)
  void OwnVertexWeights(format::Array<Weight> **table, size_t count) {
    release_weights_ = [table, count]() {
      for (size_t i = 0; i < count; i++) delete table[i];
      delete[] table;
    };
  }

  VertexID n_ = 0;
  NumEdges m_ = 0;
  NumEdges ncon_ = 0;  // number of vertex weights
  format::Array<Weight> **vertexWeights_ = nullptr;

 private:
  void Adopt(format::Format *conn) {
    this->set_connectivity(conn, true);
    this->VerifyStructure();
    InitializeInfoFromConnection();
  }
  std::function<void()> release_weights_;
};

template <typename VertexID, typename NumEdges, typename Weight>
class HyperGraph : public Graph<VertexID, NumEdges, Weight> {
 public:
  HyperGraph() = default;
  HyperGraph(format::Format *connectivity, VertexID base_type, VertexID constraint_num,
             format::CSR<VertexID, NumEdges, Weight> *xNetCSR)
      : Graph<VertexID, NumEdges, Weight>(connectivity), constraint_num_(constraint_num), base_type_(base_type),
        xNetCSR_(xNetCSR) {}
  HyperGraph(format::Format *connectivity, format::Array<Weight> *netWeights, format::Array<Weight> *cellWeights,
             VertexID base_type, VertexID constraint_num, format::CSR<VertexID, NumEdges, Weight> *xNetCSR)
      : Graph<VertexID, NumEdges, Weight>(connectivity), constraint_num_(constraint_num), base_type_(base_type),
        xNetCSR_(xNetCSR), netWeights_(netWeights), cellWeights_(cellWeights) {}
  HyperGraph(const HyperGraph &) = delete;  // (the parts are raw pointers: a copy would share or leak them)
  HyperGraph &operator=(const HyperGraph &) = delete;
  ~HyperGraph() override {
    if (!owns_parts_) return;
    delete xNetCSR_;
    delete xNetHIPCSR_;
    if constexpr (!std::is_same_v<Weight, void>) {
      delete netWeights_;
      delete cellWeights_;
    }
  }
  // the HyperGraph frees xNetCSR_ / xNetHIPCSR_ and the two weight arrays when it dies (what a reader allocated for it)
  void OwnParts() { owns_parts_ = true; }
  bool PartsAreOwned() const { return owns_parts_; }

  VertexID constraint_num_ = 1;
  VertexID base_type_ = 0;
  format::CSR<VertexID, NumEdges, Weight> *xNetCSR_ = nullptr;
  format::Array<Weight> *netWeights_ = nullptr;
  format::Array<Weight> *cellWeights_ = nullptr;
  format::HIPCSR<VertexID, NumEdges, Weight> *xNetHIPCSR_ = nullptr;

 private:
  bool owns_parts_ = false;
};

}  // namespace sparsebase::object
#endif
